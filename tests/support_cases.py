"""The case table of tests/test_gpu_support_shapes.py -- the kernels around the five large families: the initial projection,
the latent map, cut / merge, the norms (csrc/misc.hip), the prior factor (csrc/prior.hip) and the posterior draws
(csrc/sample.hip) -- with the problems and their references, shared with tests/test_support_shapes_host.py, which checks
without a GPU that the table has a case on each side of every edge the sources define, that every exact case is exact
and that every measured reference is conditioned for its allowance.

Every edge is read from the source, so a retune moves the cases with it.  Exact cases take counts for y, integers in
[-8, 8] for the norms and multiples of 2^-8 of magnitude at most 4 everywhere else: no sum over them rounds in any order.
"""
import os
import re

import numpy as np

import support_numpy as S
from oracle import vlgp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(name):
    return open(os.path.join(ROOT, "vlgp_amd", "csrc", name)).read()


def _define(text, name):
    return int(eval(re.search(r"#define %s \(?([0-9* ]+)\)?" % name, text).group(1)))


def compiled_edges():
    """The constants the launchers of misc.hip, prior.hip and ctx.h decide by."""
    misc, prior, ctx = _src("misc.hip"), _src("prior.hip"), _src("ctx.h")
    grid = re.search(r"static inline int grid_for\(int64_t n\) \{\s*int64_t g = \(n \+ 255\) / 256;\s*if \(g > (\d+)\) g = \1;", misc)
    return dict(
        PROJ_ROWS=_define(misc, "PROJ_ROWS"),
        PROJ_THREADS=int(re.search(r"hipLaunchKernelGGL\(project_kernel, dim3\(G\), dim3\((\d+)\)", misc).group(1)),
        MAP_LT=sorted(int(v) for v in re.findall(r"if \(L <= (\d+)\) hipLaunchKernelGGL\(\(latent_map_kernel_t<\1>\)", misc)),
        GRID_MAX=int(grid.group(1)),
        NORMS_PER_WG=int(re.search(r"int g = \(int\)\(\(n \+ (\d+)\) / (\d+)\);", misc).group(2)),
        PRIOR_SLOTS=_define(ctx, "VLGP_PRIOR_SLOTS"),
        # launch_ichol_all: the one-wave kernel and the workgroup of 64, of 256, of 1024; scratch in LDS or global
        ICH_T_WAVE=int(re.search(r"else if \(pr\.T <= (\d+)\) CHK\(launch_ichol_t<64>", prior).group(1)),
        ICH_T_256=int(re.search(r"else if \(pr\.T <= (\d+)\) CHK\(launch_ichol_t<256>", prior).group(1)),
        ICH_T_LDS=int(re.search(r"const bool in_lds = pr\.T <= (\d+);", prior).group(1)),
        ICH_LEAVES=tuple(int(v) for v in re.search(r"#define ICH_LEAVES\(T\) \(\(T\) / (\d+) \+ (\d+)\)", prior).groups()),
    )


E = compiled_edges()
LDS_DEFAULT = 64 * 1024  # a kernel's dynamic LDS without hipFuncSetAttribute
LDS_CU = 160 * 1024      # what a workgroup can ask of a compute unit at all


def dyadic(rng, shape):
    """Multiples of 2^-8 in [-4, 4]."""
    return rng.integers(-1024, 1025, shape).astype(np.float64) / 256.0


def _seed(cid):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(cid))


def _freeze(obj):
    for v in (obj.values() if isinstance(obj, dict) else obj):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, (dict, list, tuple)):
            _freeze(v)
    return obj


# ---- a. initial projection ---------------------------------------------------------------------------------------------
def project_lds(N):
    """launch_project's request: PROJ_ROWS rows of N | 1 doubles."""
    return E["PROJ_ROWS"] * (N | 1) * 8


PROJECT_N_64K = max(N for N in range(1, 4096) if project_lds(N) <= LDS_DEFAULT)  # the last N under the default ceiling
PROJECT_N_MAX = max(N for N in range(1, 4096) if project_lds(N) <= LDS_CU)       # the last N a CU can grant: see build_project


def project_case(cid, N, L, rows, real=False):
    rpw = E["PROJ_ROWS"]
    lds = project_lds(N)
    return dict(id=cid, N=N, L=L, rows=rows, real=real, rpw=rpw, G=-(-rows // rpw), lds=lds, raised=lds > LDS_DEFAULT)


def build_project():
    # launch_project has no cap on its LDS request: above PROJECT_N_MAX channels it asks for more than a CU has and the
    # launch is expected to return an error status.  The cases stop at that size (the defect is open).
    R, rows = E["PROJ_ROWS"], 2 * E["PROJ_ROWS"] + 2
    ns = sorted({1, 2, R - 1, R, PROJECT_N_64K, PROJECT_N_64K + 1, PROJECT_N_64K + 2, PROJECT_N_MAX})
    m = [project_case("a-N%d" % N, N, 4, rows) for N in ns]
    m += [project_case("a-rows%d" % r, 20, 4, r) for r in (1, R - 1, R, R + 1)]
    m += [project_case("a-rows%d-G%d" % (R * G + 5, G + 1), 20, 4, R * G + 5) for G in (1, 2, 3, 4, 7)]
    m += [project_case("a-L%d" % L, 20, L, rows) for L in (1, E["PROJ_THREADS"] // R + 1, 64)]  # R L below and above the threads
    m.append(project_case("a-real-N%d" % (PROJECT_N_64K + 2), PROJECT_N_64K + 2, 4, rows, real=True))
    return m


def project_problem(c, seed=None):
    rng = np.random.default_rng(_seed(c["id"]) if seed is None else seed)
    shape = (c["N"], c["L"])
    if c["real"]:
        y = rng.poisson(1.5, (c["rows"], c["N"])).astype(float)
        return y, rng.standard_normal(shape), rng.standard_normal(c["L"])
    y = rng.poisson(2.0, (c["rows"], c["N"])).astype(float)
    return y, dyadic(rng, shape), dyadic(rng, c["L"])


# ---- b. latent map -----------------------------------------------------------------------------------------------------
def map_class(L):
    for lt in E["MAP_LT"]:
        if L <= lt:
            return lt
    return 0  # the loop form


def grid_trips(n):
    """Trips of the grid-stride loop of a 256-thread kernel launched by grid_for(n)."""
    g = min(max(-(-n // 256), 1), E["GRID_MAX"])
    return -(-n // (g * 256))


def map_case(cid, L, rows, shift=True, real=False):
    return dict(id=cid, L=L, rows=rows, shift=shift, real=real, LT=map_class(L), trips=grid_trips(rows))


BIG_ROWS = E["GRID_MAX"] * 256 + 1


def build_map():
    m = []
    for L in sorted({1, 64} | set(E["MAP_LT"]) | {lt + 1 for lt in E["MAP_LT"]}):  # every template exact and one past it
        m.append(map_case("b-L%d-shift" % L, L, 257))
        m.append(map_case("b-L%d-noshift" % L, L, 257, shift=False))
    padded = E["MAP_LT"][0] + 1  # a padded L of the second template
    m += [map_case("b-rows%d" % r, padded, r) for r in (1, 255, 256)]
    m += [map_case("b-stride-L%d" % L, L, BIG_ROWS) for L in (1, padded)]
    m.append(map_case("b-real-L%d" % (E["MAP_LT"][1] + 1), E["MAP_LT"][1] + 1, 257, real=True))
    return m


def map_problem(c):
    rng = np.random.default_rng(_seed(c["id"]))
    L = c["L"]
    if c["real"]:
        return rng.standard_normal((c["rows"], L)), rng.standard_normal((L, L)), rng.standard_normal(L)
    mat = dyadic(rng, (L, L))
    assert L == 1 or not np.array_equal(mat, mat.T)
    return dyadic(rng, (c["rows"], L)), mat, dyadic(rng, L) if c["shift"] else None


OVERLAP_L = (2, 17)  # overlapping segments: the loop form of links_map_kernel at a small L and past the last template


# ---- c. cut and merge --------------------------------------------------------------------------------------------------
def cut_case(cid, N, L, P, rows, window, starts):
    starts = [int(s) for s in starts]
    srt = sorted(starts)
    disjoint = all(starts[k] >= starts[k - 1] + window for k in range(1, len(starts)))  # launch_scatter's own test
    tiling = starts == [k * window for k in range(len(starts))] and len(starts) * window == rows
    assert all(0 <= s and s + window <= rows for s in starts) and not tiling
    return dict(id=cid, N=N, L=L, P=P, rows=rows, window=window, starts=starts, one_launch=disjoint,
                overlapping=any(b < a + window for a, b in zip(srt, srt[1:])),
                y_trips=grid_trips(len(starts) * window * N))


def build_cut():
    m = []
    for P in (1, 2, 3):
        m.append(cut_case("c-P%d" % P, 7, 3, P, 300, 50, (0, 60, 130, 250)))       # disjoint, not tiling
    for N in (1, 65):
        m.append(cut_case("c-N%d" % N, N, 2, 2, 120, 25, (5, 30, 95)))
    for window in (1, 2, 50):
        m.append(cut_case("c-window%d" % window, 5, 3, 2, 200, window, (3, 3 + window, 100, 200 - window)))
    m.append(cut_case("c-one-unit", 5, 3, 2, 90, 40, (17,)))
    rows = 20000                                                                    # y: 64 * 19 950 > GRID_MAX * 256 elements
    m.append(cut_case("c-stride", 64, 2, 1, rows, 50, tuple(range(25, rows - 50, 50))))
    m.append(cut_case("c-overlap-sorted", 5, 3, 2, 200, 50, (0, 30, 60, 150)))
    m.append(cut_case("c-overlap-equal", 5, 3, 2, 200, 50, (10, 40, 40, 120)))
    m.append(cut_case("c-overlap-unsorted", 5, 3, 2, 200, 50, (120, 0, 100, 20, 100)))
    return m


def cut_problem(c):
    """y counts; x real (dyadic, never all ones); mu, v, w dyadic; the segments' new (mu, v) a merge writes back."""
    rng = np.random.default_rng(_seed(c["id"]))
    rows, N, L, P = c["rows"], c["N"], c["L"], c["P"]
    p = dict(y=rng.poisson(1.0, (rows, N)).astype(float), x=dyadic(rng, (rows, P, N)),
             mu=dyadic(rng, (rows, L)), v=dyadic(rng, (rows, L)) + 5.0, w=dyadic(rng, (rows, L)) + 5.0)
    n_seg = len(c["starts"]) * c["window"]
    p["new_mu"], p["new_v"] = dyadic(rng, (n_seg, L)), dyadic(rng, (n_seg, L)) + 5.0
    p["proj"], p["shift"] = dyadic(rng, (N, L)), dyadic(rng, L)
    p["a"], p["b"] = 0.25 * dyadic(rng, (L, N)), 0.25 * dyadic(rng, (P, N))
    return _freeze(p)


# ---- d. norms ----------------------------------------------------------------------------------------------------------
NORMS_DEFAULT_BLOCKS = 256


def norms_case(n, blocks=None):
    g = min(max(-(-n // E["NORMS_PER_WG"]), 1), blocks or NORMS_DEFAULT_BLOCKS)
    per_trip = g * E["NORMS_PER_WG"]  # 256 lanes x 4 strided loads per workgroup and trip
    tail = n - (n - 1) // per_trip * per_trip  # elements of the last trip
    return dict(id="d-n%d-%s" % (n, "default" if blocks is None else "blocks%d" % blocks), n=n, blocks=blocks, g=g,
                trips=-(-n // per_trip), loads_in_range=-(-tail // (g * 256)), fold_trips=-(-g // 256))


def build_norms():
    W = E["NORMS_PER_WG"]
    m = [norms_case(n) for n in (1, 255, 256, 257, W - 1, W, W + 1, NORMS_DEFAULT_BLOCKS * W + 1)]
    m += [norms_case(n, 1) for n in (W, W + 1, 2 * W + 1)]
    m += [norms_case(n, 7) for n in (7 * W, 7 * W + 1, 2 * 7 * W + 769)]
    m.append(norms_case(1024 * W + 1, 1024))
    return m


def norms_problem(c):
    return _freeze([np.random.default_rng(_seed(c["id"])).integers(-8, 9, (c["n"], 1)).astype(np.float64)])[0]


# ---- e. prior factor ---------------------------------------------------------------------------------------------------
def prior_lds(T):
    """Dynamic LDS of ichol_exact_kernel with residuals, kernel values and pivots in LDS (launch_ichol_all, csrc/prior.hip)."""
    NL = T // E["ICH_LEAVES"][0] + E["ICH_LEAVES"][1]
    return 8 * (16 + NL + 2 * T) + 4 * (24 + 2 * NL + T) + 16


T_E = next(T for T in range(E["ICH_T_256"] + 1, E["ICH_T_LDS"] + 1) if prior_lds(T) > LDS_DEFAULT)  # first raised ceiling


def prior_plan(T, R, block=False):
    """The launch csrc/prior.hip's launch_ichol_all chooses for a length, restated from its conditions."""
    wave = T <= E["ICH_T_WAVE"] and not block
    glob = T > E["ICH_T_LDS"]
    if wave:
        lds = 8 * (T * (R | 1) + 128) + 4 * 64
    elif glob:
        NL = T // E["ICH_LEAVES"][0] + E["ICH_LEAVES"][1]
        lds = 8 * (16 + NL) + 4 * (24 + 2 * NL) + 16
    else:
        lds = prior_lds(T)
    nt = 64 if T <= E["ICH_T_WAVE"] else 256 if T <= E["ICH_T_256"] else 1024
    return dict(wave=int(wave), nt=nt, lds=lds, raised=int(lds > LDS_DEFAULT), global_scratch=int(glob), rs=R | 1)


def smooth(T):
    return (6.0 / max(T, 8)) ** 2


# 128, 129, 136, 137, 256, 257, 1024, 1025: NumPy's pairwise sum (leaves of 128, halves rounded to 8), not the launcher's
LENGTHS = tuple(sorted({1, E["ICH_T_WAVE"] + 1, 128, 129, 136, 137, 256, 257, E["ICH_T_256"], E["ICH_T_256"] + 1, 1024, 1025,
                        T_E - 1, T_E, E["ICH_T_LDS"], E["ICH_T_LDS"] + 1, E["ICH_T_LDS"] + 904}))
T_SHORT, T_MID, T_LONG = E["ICH_T_WAVE"] + 1, E["ICH_T_256"] + 1, E["ICH_T_LDS"] + 1  # the first length of each class
ROUGH = 0.7


def prior_case(cid, lengths, R, omega, sigma, rebuild=None, kinds=None):
    return dict(id=cid, lengths=list(lengths), R=R, L=len(omega), omega=np.array(omega, dtype=float),
                sigma=np.array(sigma, dtype=float), rebuild=None if rebuild is None else np.array(rebuild, dtype=float),
                kinds=kinds)


def build_prior():
    m = []
    for T in LENGTHS:  # one smooth latent that stops on the tolerance, one rough that fills R columns
        m.append(prior_case("e-T%d" % T, [T], 50, (smooth(T), ROUGH), (1.0, 0.75), kinds=("smooth", "rough")))
    for R in (1, 50, 64):
        for T in (T_SHORT, T_MID):
            m.append(prior_case("e-R%d-T%d" % (R, T), [T], R, (smooth(T), 2.5), (1.25, 1.0), kinds=("smooth", "rough")))
    grid16 = np.exp(np.linspace(np.log(2e-4), np.log(3.0), 16))
    for T in (T_SHORT, T_LONG):
        m.append(prior_case("e-L16-T%d" % T, [T], 50, grid16, 0.5 + np.arange(16) / 16.0))
        m.append(prior_case("e-L1-T%d" % T, [T], 50, (0.5,), (1.5,)))
    for n in (E["PRIOR_SLOTS"] + 1, 2 * E["PRIOR_SLOTS"] + 2):  # a second and a third mailbox round
        m.append(prior_case("e-%dlengths" % n, range(141 - n, 141), 50, (1e-3, 2e-2), (1.0, 2.0)))
    for n in (E["PRIOR_SLOTS"], E["PRIOR_SLOTS"] + 1):  # rebuilt in place: ranks deferred at 64 lengths, waited for at 65
        m.append(prior_case("e-rebuild-%dlengths" % n, range(141 - n, 141), 50, (1e-3, 2e-2), (1.0, 2.0), rebuild=(3e-2, 5e-4)))
    return m


_factors = {}


def oracle_factor(T, omega, sigma, R):
    """(G (T, R), rank) of one latent: the oracle's bits."""
    key = (int(T), float(omega), float(sigma), int(R))
    if key not in _factors:
        G = O.ichol_gauss(int(T), float(omega), int(R)) * float(sigma)
        G.setflags(write=False)
        _factors[key] = (G, int((np.abs(G).sum(0) > 0).sum()))
    return _factors[key]


COMPACT = [dict(id="e-compact-T%d" % T, T=T, L=3, R=50, N=6, omega=np.array([smooth(T), 4.0 * smooth(T), ROUGH]),
                sigma=np.array([1.0, 0.8, 1.2])) for T in (T_SHORT, T_MID)]


def injected_factors():
    """(id, G (L, T, R), ranks) for set_prior: interior zero column, all zero, only the last entry, one bin."""
    rng = np.random.default_rng(5)
    out = []
    T, R = 37, 12
    G = np.zeros((3, T, R))
    G[0, :, :7] = rng.standard_normal((T, 7))
    G[0, :, 3] = 0.0                      # interior zero column, later ones set: rank 7
    G[2, T - 1, R - 1] = 0.5              # only the last entry: rank R; latent 1 all zero: rank 1
    out.append(("e-inject-T37", G, [7, 1, R]))
    G1 = np.zeros((3, 1, R))
    G1[0, 0, 0] = 1.0
    G1[1, 0, 4] = -2.0
    out.append(("e-inject-T1", G1, [1, 5, 1]))
    big = np.zeros((2, 300, 50))          # more than 256 entries per thread stride, the last column on one late row only
    big[0, :, :20] = rng.standard_normal((300, 20))
    big[0, 299, 49] = 1e-300
    big[1, 0, 0] = 1.0
    out.append(("e-inject-T300", big, [50, 1]))
    return out


# ---- f. posterior draws ------------------------------------------------------------------------------------------------
def draw_case(cid, T, R, n, omega, w="random", factor="ichol", compare="measured"):
    return dict(id=cid, T=T, R=R, n=n, L=len(omega), omega=tuple(omega), w=w, factor=factor, compare=compare)


def build_draws():
    m = [draw_case("f-R%d" % R, 70, R, 16, (5e-3, 1.0)) for R in (1, 2, 50, 64)]  # the rough latent fills R columns
    m.append(draw_case("f-rank1-beside-full", 40, 8, 16, (0.0, 1.0)))  # K = 11': one column
    m.append(draw_case("f-r64-T70", 70, 64, 16, (1.0,)))
    m.append(draw_case("f-zero-factor", 30, 50, 16, (1e-2, 1e-2), factor="zero", compare="bits"))
    m += [draw_case("f-T%d" % T, T, 50, 16, (2e-3, 3e-2)) for T in (1, 2, 257)]
    m += [draw_case("f-n%d" % n, 30, 50, n, (5e-3, 5e-2)) for n in (1, 255, 256, 257, 1000)]
    m.append(draw_case("f-w0", 40, 50, 16, (5e-3, 5e-2), w="zero", compare="bound"))
    m.append(draw_case("f-w1e6", 40, 50, 16, (5e-3, 2e-2), w="spikes"))
    return m


FLOOR = 64 * S.U
ALLOWANCE_CAP = 1e-10  # the tolerance of tests/test_gpu_branches.py::test_sample_posterior_on_the_device


def rel_distance(got, want):
    want = np.asarray(want, dtype=np.longdouble)
    return float(np.max(np.abs(np.asarray(got, dtype=np.longdouble) - want)) / np.max(np.abs(want)))


_draws = {}


def draw_problem(cid):
    """(problem, reference): mu, w (T, L), G (L, T, R), eps (L, R, n); `want` the longdouble statement, `ranks`, and for a
    measured case `allowance` = max(16 x the float64 oracle's distance from the statement, FLOOR), relative to max |want|."""
    if cid in _draws:
        return _draws[cid]
    c = DRAW_BY_ID[cid]
    rng = np.random.default_rng(_seed(cid))
    T, L, R, n = c["T"], c["L"], c["R"], c["n"]
    if c["factor"] == "zero":
        G = np.zeros((L, T, R))
    else:
        G = np.stack([oracle_factor(T, om, 0.8 + 0.4 * l, R)[0] for l, om in enumerate(c["omega"])])
    mu = rng.standard_normal((T, L))
    w = {"random": 0.2 + rng.random((T, L)), "zero": np.zeros((T, L)), "spikes": 0.2 + rng.random((T, L))}[c["w"]]
    if c["w"] == "spikes":
        w[rng.choice(T, 3, replace=False)] = 1e6
    eps = rng.standard_normal((L, R, n))
    p = dict(mu=mu, w=w, G=G, eps=eps, ranks=[S.factor_rank(G[l]) for l in range(L)])
    ref = dict(want=S.sample_posterior(mu, w, G, eps))
    if c["compare"] == "measured":
        orc = O.sample_posterior_lowrank(mu, w, G, [eps[l, :r] for l, r in enumerate(p["ranks"])])
        ref["oracle_distance"] = rel_distance(orc, ref["want"])
        ref["allowance"] = max(16.0 * ref["oracle_distance"], FLOOR)
    elif c["compare"] == "bound":
        ref["bound"] = S.draw_bound_w0(mu, G, eps)
    _draws[cid] = (_freeze(p), _freeze(ref))
    return _draws[cid]


PROJECT, MAP, CUT, NORMS, PRIOR, DRAWS = build_project(), build_map(), build_cut(), build_norms(), build_prior(), build_draws()
ALL = PROJECT + MAP + CUT + NORMS + PRIOR + DRAWS
assert len({c["id"] for c in ALL}) == len(ALL)
PROJECT_BY_ID, MAP_BY_ID, CUT_BY_ID = ({c["id"]: c for c in m} for m in (PROJECT, MAP, CUT))
NORMS_BY_ID, PRIOR_BY_ID, DRAW_BY_ID = ({c["id"]: c for c in m} for m in (NORMS, PRIOR, DRAWS))
