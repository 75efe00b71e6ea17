"""vlgp_amd/csrc/fast_exp.h -- the five exponentials every Poisson rate of the E- and M-step goes through -- compiled
for the CPU (tests/native/fast_exp_harness.cpp behind tests/native/hip_shim, g++) and held ELEMENT BY ELEMENT to the
accuracy the header documents, over the whole domain.  No GPU needed; tests/test_gpu_rates.py runs the same checks on
the device build (probe kinds 4 ... 8 of vlgp_debug_npx) and on the copies inlined into the real kernels.

  kind 4  fast_exp(clamp10(x))               estep_fast / estep_long / M-step rate cache     "< 2 ulp"
  kind 5  fast_exp_tab<false>(clamp10(x))    64-entry table                                  "< 1.5 ulp"
  kind 6  trunc_exp_tab64(x)                 M-step Newton pass                              "< 1.5 ulp"
  kind 7  fast_exp_tab256<false>(clamp10(x)) 256-entry table                                 "< 1.5 ulp"
  kind 8  trunc_exp_tab256(x)                estep_split row passes (the headline path)      "< 1.5 ulp"

Reference: exp from the standard library's `decimal` at 60 digits; the error of a result is |got - exact| in units of
the last place of the EXACT value (2^-1074 where the exact value is subnormal), computed in 60-digit decimal arithmetic.

Special values, pinned as they are today (three-way table; the reference is math.trunc_exp, vlgp/math.py:24-38,
exp(min(x, 10))):

            reference   fast_exp(clamp10(.)), fast_exp_tab*<false>(clamp10(.))   trunc_exp_tab64 / 256
    NaN     NaN         NaN                                                      NaN
    +inf    exp(10)     exp(10)                                                  NaN
    -inf    0           2^-1074 (the value at -745)                              NaN

(No finite input reaches an infinite linear predictor: every update of the E- and M-step is clipped.)

Known edge, not changed here: `y log(rate)` in csrc/evaluate.hip is NaN for y = 0 once eta < -745.13 (the rate
underflows to 0); no fit reaches that.
"""
import ctypes as C
import math
import os
import subprocess
import tempfile
from decimal import Context, Decimal

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

KINDS = {4: "fast_exp(clamp10)", 5: "fast_exp_tab<false>(clamp10)", 6: "trunc_exp_tab64",
         7: "fast_exp_tab256<false>(clamp10)", 8: "trunc_exp_tab256"}
# the bounds fast_exp.h documents, in ulp
BOUND = {4: 2.0, 5: 1.5, 6: 1.5, 7: 1.5, 8: 1.5}
FAST_KINDS, TRUNC_KINDS = (4, 5, 7), (6, 8)
DENORMAL_BOUND = 1.0  # units of 2^-1074 on [-745.13, -708.4]: the result is rounded once more by ldexp

CTX = Context(prec=60)
LN2 = CTX.ln(Decimal(2))
EXP10 = float(CTX.exp(Decimal(10)))  # correctly rounded exp(10)
TINY = 2.0 ** -1074


# ---------------------------------------------------------------------------------------------------------------------
# the CPU build of the header
class Harness:
    def __init__(self):
        out = os.path.join(tempfile.mkdtemp(prefix="fx_"), "libfx.so")
        native = os.path.join(HERE, "native")
        subprocess.run(["g++", "-O2", "-mfma", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC",
                        "-I" + os.path.join(native, "hip_shim"), os.path.join(native, "fast_exp_harness.cpp"),
                        "-o", out], check=True)
        self.lib = C.CDLL(out)
        self.lib.fx_eval.restype = C.c_int

    def __call__(self, kind, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty_like(x)
        rc = self.lib.fx_eval(int(kind), x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), C.c_long(x.size))
        assert rc == 0, kind
        return y

    def tables(self):
        t = [np.empty(64), np.empty(256), np.empty(64), np.empty(256)]
        self.lib.fx_tables(*[a.ctypes.data_as(C.c_void_p) for a in t])
        return t


@pytest.fixture(scope="module")
def fx():
    return Harness()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# the exact reference
_POW2 = {}


def _pow2(e):
    """2^e as a 60-digit decimal"""
    if e not in _POW2:
        _POW2[e] = CTX.power(Decimal(2), Decimal(e))
    return _POW2[e]


class Reference:
    """exp(min(x, 10)) of every element of a finite array to 60 digits, and the unit in the last place of each exact
    value (2^-1074 in the subnormal range).  `ulp_error(got)` is |got - exact| / ulp, element by element."""

    def __init__(self, x):
        self.x = np.ascontiguousarray(x, dtype=np.float64)
        assert np.all(np.isfinite(self.x))
        self.exact, self.inv_ulp = [], []
        ten = Decimal(10)
        for v in self.x.tolist():
            d = Decimal(v)
            e = CTX.exp(d if d < ten else ten)
            f = float(e)  # correctly rounded
            ex = math.frexp(f)[1] if f > 0.0 else -1100  # f = m 2^ex, 1/2 <= m < 1
            if f > 0.0 and Decimal(f) > e and math.frexp(f)[0] == 0.5:
                ex -= 1  # the exact value lies below the power of two it rounds to
            self.exact.append(e)
            self.inv_ulp.append(_pow2(-max(ex - 53, -1074)))
        self.rounded = np.array([float(e) for e in self.exact])

    def ulp_error(self, got):
        got = np.ascontiguousarray(got, dtype=np.float64)
        assert got.shape == self.x.shape
        err = np.empty(got.size)
        for i, g in enumerate(got.tolist()):
            if not math.isfinite(g):
                err[i] = math.inf
            else:
                err[i] = float(CTX.multiply(abs(CTX.subtract(Decimal(g), self.exact[i])), self.inv_ulp[i]))
        return err


def worst(ref, got):
    """(largest error in ulp, the input where it occurs)"""
    err = ref.ulp_error(got)
    i = int(np.argmax(err))
    return float(err[i]), float(ref.x[i])


# ---------------------------------------------------------------------------------------------------------------------
# the designed sample
def _neighbours(c):
    c = np.asarray(c, dtype=np.float64)
    return np.concatenate([np.nextafter(c, -np.inf), c, np.nextafter(c, np.inf)])


def cell_points(entries):
    """For every index j of the `entries`-entry table, at several binary exponents e of the result -- the smallest
    normal (-1022), two mid-range ones, -1, 0 and the largest whose cell lies below the clamp at 10 -- the cell centre
    k ln2/entries, k = entries e + j, and both cell edges (k +- 1/2) ln2/entries, each with its two neighbouring
    doubles: where |r| is largest and where the rounding of k flips."""
    pts = []
    for j in range(entries):
        top = int(math.floor((10.0 * entries / math.log(2.0) - j - 0.5) / entries))
        while (2 * (entries * top + j) + 1) * LN2 / (2 * entries) > 10:
            top -= 1
        for e in (-1022, -700, -37, -1, 0, top):
            k = entries * e + j
            for num in (2 * k - 1, 2 * k, 2 * k + 1):
                pts.append(float(CTX.divide(CTX.multiply(Decimal(num), LN2), Decimal(2 * entries))))
    return _neighbours(np.array(pts))


def designed_sample(seed=20240611):
    """Tens of thousands of points of [-709, 10]: uniform draws on [-30, 10], [-708, -30] and [-1e-3, 1e-3], and the
    cell centres / edges of both tables (cell_points).  Finite, at most 10, results normal or just below."""
    rng = np.random.default_rng(seed)
    parts = [rng.uniform(-30.0, 10.0, 20000), rng.uniform(-708.0, -30.0, 20000), rng.uniform(-1e-3, 1e-3, 20000),
             cell_points(256), cell_points(64), np.array([0.0, -0.0, 10.0, np.nextafter(10.0, 0.0), 1.0, -1.0])]
    return np.concatenate(parts)


def denormal_sample(seed=7):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-745.13, -708.4, 6000), np.array([-745.13, -745.0, -744.5, -708.4, -709.0])])


_REF_CACHE = {}


def reference_for(name):
    """Reference of the designed / the denormal sample (built once per process: ~80 000 60-digit exponentials)."""
    if name not in _REF_CACHE:
        _REF_CACHE[name] = Reference(designed_sample() if name == "designed" else denormal_sample())
    return _REF_CACHE[name]


# ---------------------------------------------------------------------------------------------------------------------
# the checks, written against any evaluator f(kind, x) -> y (the CPU harness here, the device probe in test_gpu_rates)
def check_accuracy(f, report=None):
    ref, den = reference_for("designed"), reference_for("denormal")
    bad = []
    for kind in KINDS:
        e, at = worst(ref, f(kind, ref.x))
        ed, atd = worst(den, f(kind, den.x))
        print("%-34s designed sample %.4f ulp at x = %r; [-745.13, -708.4] %.4f x 2^-1074 at x = %r"
              % (KINDS[kind], e, at, ed, atd))
        if report is not None:
            report[kind] = (e, ed)
        if not e < BOUND[kind]:
            bad.append((KINDS[kind], "designed", e, at))
        if not ed <= DENORMAL_BOUND:
            bad.append((KINDS[kind], "denormal", ed, atd))
    assert not bad, bad


def check_clamp(f):
    above = np.array([10.0, np.nextafter(10.0, 11.0), 11.0, 700.0, 1e300])
    below10 = np.array([np.nextafter(10.0, 0.0)])
    under = np.array([np.nextafter(-745.0, -746.0), -745.13, -745.2, -746.0, -1e4, -1e300])
    for kind in KINDS:
        at10 = f(kind, np.array([10.0]))[0]
        assert abs(at10 - EXP10) <= BOUND[kind] * np.spacing(EXP10), KINDS[kind]
        assert np.array_equal(bits(f(kind, above)), bits(np.full(above.size, at10))), KINDS[kind]
        # the double below 10 (10 - 2^-49) is NOT clamped: its own value, ~11 ulp below exp(10)
        lo = f(kind, below10)[0]
        assert lo < at10 and abs(lo - EXP10 * (1.0 - 2.0 ** -49)) <= (BOUND[kind] + 1) * np.spacing(EXP10), KINDS[kind]
        at745 = f(kind, np.array([-745.0]))[0]
        assert at745 == TINY, (KINDS[kind], at745)
        assert np.array_equal(bits(f(kind, under)), bits(np.full(under.size, at745))), KINDS[kind]


def check_special(f):
    """The three-way table of the module docstring, as it is today."""
    x = np.array([np.nan, np.inf, -np.inf])
    for kind in FAST_KINDS:
        got = f(kind, x)
        assert np.isnan(got[0]), KINDS[kind]
        assert got[1] == f(kind, np.array([10.0]))[0] and got[2] == TINY, (KINDS[kind], got)
    for kind in TRUNC_KINDS:
        assert np.all(np.isnan(f(kind, x))), (KINDS[kind], f(kind, x))
    # a NaN anywhere in an array leaves its neighbours alone
    y = np.array([0.0, np.nan, 1.0, -3.0])
    for kind in KINDS:
        got = f(kind, y)
        assert np.isnan(got[1]) and np.all(np.isfinite(got[[0, 2, 3]])) and got[0] == 1.0, KINDS[kind]


MONOTONE_POINTS = 2_000_000


def monotone_grid():
    """Sorted, ~7 points per cell of the 256-entry table (cell width ln2/256 = 2.7e-3, step 3.8e-4) from below the lower
    clamp to above the upper one: every cell boundary of both tables has grid points on either side, one step apart --
    a step changes exp by 3.8e-4 relative, thirteen orders above the rounding error, and a table index taken from the
    wrong side of a boundary would drop the value by 2^(1/256) - 1 = 2.7e-3."""
    return np.linspace(-745.5, 10.5, MONOTONE_POINTS)


def check_monotone(f):
    x = monotone_grid()
    assert np.all(np.diff(x) > 0) and np.diff(x).max() < math.log(2.0) / 256 / 4
    for kind in KINDS:
        y = f(kind, x)
        d = np.diff(y)
        assert np.all(d >= 0), (KINDS[kind], x[:-1][d < 0][:5])
        inside = (x > -700.0) & (x < 10.0)  # strictly, where neither a clamp nor the subnormal range flattens the steps
        assert np.all(d[inside[1:] & inside[:-1]] > 0), KINDS[kind]


# ---------------------------------------------------------------------------------------------------------------------
def test_tables_are_correctly_rounded_powers_of_two(fx):
    t64, t256, lds64, lds256 = fx.tables()
    want64 = np.array([float(CTX.exp(CTX.divide(CTX.multiply(Decimal(j), LN2), Decimal(64)))) for j in range(64)])
    want256 = np.array([float(CTX.exp(CTX.divide(CTX.multiply(Decimal(j), LN2), Decimal(256)))) for j in range(256)])
    assert np.array_equal(bits(t64), bits(want64)), np.nonzero(t64 != want64)[0]
    assert np.array_equal(bits(t256), bits(want256)), np.nonzero(t256 != want256)[0]
    assert np.array_equal(bits(t64), bits(t256[::4]))
    # what fast_exp_tab_init / fast_exp_tab256_init leave in the workgroup's copy
    assert np.array_equal(bits(lds64), bits(t64)) and np.array_equal(bits(lds256), bits(t256))


def test_reference_is_self_consistent():
    """The 60-digit reference against values known in closed form, and its ulp against np.spacing."""
    r = Reference(np.array([0.0, 1.0, -745.0, 10.0, 700.0, math.log(2.0), -708.0]))
    assert r.rounded[0] == 1.0 and r.rounded[1] == math.e and r.rounded[2] == TINY and r.rounded[3] == r.rounded[4] == EXP10
    assert r.ulp_error(r.rounded).max() <= 0.5
    one_up = np.nextafter(r.rounded, np.inf)
    e = np.delete(r.ulp_error(one_up), 5)  # (index 5 rounds to 2.0, whose upper neighbour is two of ITS ulps away)
    assert np.all((e >= 0.5) & (e <= 1.5))
    # exp(ln2 rounded down) is just below 2: its ulp is that of [1, 2), half of np.spacing(2.0)
    assert float(r.inv_ulp[5]) == 2.0 ** 52


def test_accuracy_on_the_designed_sample(fx):
    """|got - exact| below the header's bound (2 / 1.5 / 1.5 / 1.5 / 1.5 ulp) at every point of the designed sample, and
    at most one unit of 2^-1074 on the subnormal range."""
    assert reference_for("designed").x.size > 60000
    check_accuracy(fx)


def test_accuracy_dense_against_numpy(fx):
    """The net for a gross error where the designed sample has no point: four million points of [-745, 10] against
    np.exp (itself below 1 ulp), bound = the header's + 1 ulp."""
    rng = np.random.default_rng(99)
    x = np.concatenate([rng.uniform(-745.0, 10.0, 3_000_000), rng.uniform(-40.0, 10.0, 1_000_000)])
    want = np.exp(x)
    ulp = np.spacing(want)
    for kind in KINDS:
        err = np.abs(fx(kind, x) - want) / ulp
        i = int(np.argmax(err))
        print("%-34s dense %.3f ulp (vs np.exp) at x = %r" % (KINDS[kind], err[i], x[i]))
        assert err[i] < BOUND[kind] + 1.0, (KINDS[kind], err[i], x[i])


def test_clamps(fx):
    check_clamp(fx)


def test_monotone_across_every_cell_boundary(fx):
    check_monotone(fx)


def test_special_values_are_pinned(fx):
    check_special(fx)
    # the reference's own values, for the table in the module docstring
    with np.errstate(invalid="ignore"):
        ref = np.exp(np.minimum(np.array([np.nan, np.inf, -np.inf]), 10))
    assert np.isnan(ref[0]) and ref[1] == EXP10 and ref[2] == 0.0
