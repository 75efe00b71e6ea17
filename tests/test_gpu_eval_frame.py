"""The optional outputs of the six scoring entry points (csrc/eval_api.hip): whichever of them a caller leaves out, the
outputs still asked for are byte for byte those of the call that asks for everything, and a full call after the whole
sequence repeats the first.  One engine, units of lengths [1, 7], N = 3, L = 2, rank 4, seeded parameters, one E-step;
the calls go through ``eng.lib``, since the ``Engine`` methods always pass some of the pointers.  No input here makes a
call fail on the device (refusals: the tests of each entry point)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_forecast import SET, _engine, _problem

pytestmark = pytest.mark.gpu

N, L, R, K = 3, 2, 4, 70  # (K: two chunks of draws, the second ragged)


def _call(eng, name, ext, eps, omit=()):
    """Entry point `name` with the outputs in `omit` passed as null: {output: array} of the others."""
    from vlgp_amd.engine import dptr, hermite_nodes, iptr

    units, rows, off = eng.sets[SET]
    out = {}

    def buf(key, *shape):
        if key in omit:
            return None
        out[key] = np.full(shape, -7.0)
        return dptr(out[key])

    n = C.c_int(-1)
    n_ref = None if "n_failed" in omit else C.byref(n)
    if name == "loglik":
        rc = eng.lib.vlgp_loglik(eng.h, SET, 1, buf("rate", rows, N), buf("sums", N, 4))
        n_ref = None
    elif name == "predictive":
        z, lwa = hermite_nodes(12)
        rc = eng.lib.vlgp_predictive(eng.h, SET, 1, len(z), dptr(z), dptr(lwa), buf("rate", rows, N), buf("lpd", rows, N),
                                     buf("sums", N, 4))
        n_ref = None
    elif name == "elbo":
        rc = eng.lib.vlgp_elbo(eng.h, SET, 1, buf("row_sums", N, 4), buf("row_ell", rows), buf("kl_terms", units, L, 4), n_ref)
    elif name == "forecast":
        lengths = np.ascontiguousarray(sorted(ext), dtype=np.int32)
        n_ext = np.ascontiguousarray([ext[int(T)].shape[1] for T in lengths], dtype=np.int32)
        G_all = np.ascontiguousarray(np.concatenate([ext[int(T)].ravel() for T in lengths]))
        total = sum(int(n_ext[list(lengths).index(T)]) for T in np.diff(np.asarray(off)))
        rc = eng.lib.vlgp_forecast(eng.h, SET, 1, len(lengths), iptr(lengths), iptr(n_ext), dptr(G_all),
                                   buf("mu_ext", total, L), buf("v_ext", total, L), buf("fit_terms", units, L, 2), n_ref)
    elif name == "marginal":
        rc = eng.lib.vlgp_marginal(eng.h, SET, 1, K, dptr(eps), buf("log_w", units, K), buf("parts", units, K, 2), n_ref)
    else:
        k = 0 if "log_w" in omit else K
        rc = eng.lib.vlgp_joint_laplace(eng.h, SET, 50, 1e-10, k, dptr(eps) if k else None, buf("beta", units, L, R),
                                        buf("stats", units, 8), buf("mu", rows, L), buf("v", rows, L),
                                        buf("log_w", units, K), buf("parts", units, K, 2), n_ref)
    eng.check(rc)
    if n_ref is not None:
        out["n_failed"] = np.array([n.value])
    return out


OMIT = {
    "loglik": [("rate",)],
    "predictive": [("rate",), ("lpd",), ("rate", "lpd")],
    "elbo": [("row_ell",), ("n_failed",), ("row_ell", "n_failed")],
    "forecast": [("fit_terms",), ("n_failed",), ("fit_terms", "n_failed")],
    "marginal": [("parts",), ("n_failed",), ("parts", "n_failed")],
    "joint_laplace": [("beta",), ("mu",), ("v",), ("mu", "v"), ("parts",), ("n_failed",), ("log_w", "parts"),
                      ("beta", "mu", "v", "log_w", "parts", "n_failed")],
}


def test_left_out_outputs_change_nothing_in_the_others():
    import vlgp_amd as V

    units, par, prior, ext = _problem([1, 7], {1: 2, 7: 3}, N, L, [2e-2, 5e-3], seed=5, R=R)
    eps = np.random.default_rng(1).standard_normal((len(units), L, R, K))
    with _engine(V, units, par, prior, R=R) as eng:
        assert eng.estep(SET, 3, 5.0, True) == 0
        full = {name: _call(eng, name, ext, eps) for name in OMIT}
        for name, out in full.items():
            assert all(np.all(np.isfinite(a)) and not np.any(a == -7.0) for a in out.values()), name
            assert "n_failed" not in out or out["n_failed"][0] == 0
        for name, omits in OMIT.items():
            for omit in omits:
                got = _call(eng, name, ext, eps, omit)
                assert sorted(got) == sorted(set(full[name]) - set(omit)), (name, omit)
                for key, arr in got.items():
                    assert arr.tobytes() == full[name][key].tobytes(), (name, omit, key)
        for name in OMIT:
            again = _call(eng, name, ext, eps)
            assert sorted(again) == sorted(full[name])
            for key, arr in again.items():
                assert arr.tobytes() == full[name][key].tobytes(), (name, key)
