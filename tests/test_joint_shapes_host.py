"""The case table of tests/joint_shapes.py on the CPU: every case has the ranks and the D it is named for, its NumPy
statement converges, and the halving case halves.  No GPU.
"""
import numpy as np
import pytest

import joint_numpy as JN
import joint_shapes as JS

NEWTON_TOL = 1e-20


@pytest.mark.parametrize("name", sorted(JS.CASES))
def test_case_has_its_ranks_and_its_statement_converges(name):
    case = JS.CASES[name]
    units, params, gauss = JS.problem(name)
    st = JS.reference(name)
    assert len(st) == len(units) == len(case["units"])
    assert len({T for T, _ in case["units"]}) == len(units)  # a length, hence a rank pattern, of its own per unit
    for u, s, (T, ranks) in zip(units, st, case["units"]):
        G = params["cholesky"][T]
        assert u["y"].shape == (T, case["N"]) and G.shape == (case["L"], T, case["R"])
        assert s["ranks"] == list(ranks) and s["unit"].D == sum(ranks)
        for l, r in enumerate(ranks):
            assert JN.rank(G[l]) == r and np.all(np.any(G[l][:, :r] != 0.0, axis=0)) and not np.any(G[l][:, r:])
            assert np.max(np.sum(G[l] ** 2, axis=1)) <= 1.0 + 1e-12
        assert s["converged"] and s["decrement"] <= NEWTON_TOL, (name, T, s["decrement"])
        assert s["halvings"] >= 0 and np.all(np.isfinite(s["log_w"])) and np.all(np.isfinite(s["cov"]))
    top = [float(np.linalg.eigvalsh(s["H"])[-1]) for s in st]
    print("joint shapes [%s] D %s newton %s halvings %s lambda_max(H) %s" % (
        name, JS.dims(name), [s["n_newton"] for s in st], [s["halvings"] for s in st], np.round(top, 1).tolist()))


def test_the_table_crosses_every_size_it_is_named_for():
    D = {name: JS.dims(name) for name in JS.CASES}
    ranks = {name: [r for _, r in JS.CASES[name]["units"]] for name in JS.CASES}
    assert D["D_255_to_288"] == [255, 256, 257, 288] and D["D_511_512_33"] == [511, 512, 33]
    assert ranks["D_511_512_33"][1] == [64] * 8
    assert any({64, 63, 1} <= set(r) for r in ranks["D_255_to_288"])
    assert D["panel_32_64_224"] == [32, 64, 224]
    c = JS.CASES["LR_512_small_D"]
    assert c["L"] * c["R"] > 256 and max(D["LR_512_small_D"]) <= 64 and max(max(r) for r in ranks["LR_512_small_D"]) == 9
    c = JS.CASES["rows_256_257_600"]
    assert [T for T, _ in c["units"]] == [256, 257, 600] and max(max(r) for _, r in c["units"]) <= 16 and c["N"] >= 65
    c = JS.CASES["L16_npair_136"]
    assert c["L"] == 16 and c["L"] * (c["L"] + 1) // 2 == 136 and c["R"] == 50
    assert {r for rk in ranks["L16_npair_136"] for r in rk} == set(range(1, 10))
    assert JS.CASES["L11_D_512"]["L"] == 11 and D["L11_D_512"][0] == 512 and max(D["L11_D_512"]) <= 512
    for name in JS.CASES:
        assert all(min(r) >= 1 for r in ranks[name]) and max(D[name]) <= 512
        if name == "late_rows_300":
            assert [T for T, _ in JS.CASES[name]["units"]] == [300, 257] and JS.CASES[name]["N"] <= 8
        elif name != "rows_256_257_600":
            assert JS.CASES[name]["N"] <= 8 and max(T for T, _ in JS.CASES[name]["units"]) <= 130
    assert set(JS.MASKED) <= set(JS.CASES)


def test_the_halving_case_rejects_a_full_step():
    st = JS.reference("halving")
    assert max(s["halvings"] for s in st) >= 1, [s["halvings"] for s in st]
    assert all(s["converged"] for s in st)


def test_the_late_rows_case_needs_every_row_in_the_decision():
    """From the same start, with the same gradient and Hessian, the iteration that judges its trial points by the first 256
    rows alone does not reach the mode of the 300-row unit in the 50 factorisations the device is given; the statement's
    does.  A device whose joint_decide stopped after one pass of its row loop would therefore fail this case."""
    units, params, gauss = JS.problem("late_rows_300")
    st = JS.reference("late_rows_300")
    u = units[0]
    U = JN.Unit(u, params["a"], params["b"], params["noise"], gauss, params["cholesky"][300])
    start = JN.mean_field_start(U, u)
    whole = JN.newton(U, start, NEWTON_TOL, 50)
    first = JN.newton(JS.DecideOnFirstRows(U), start, NEWTON_TOL, 50)
    assert whole[3] and whole[2] == st[0]["n_newton"] <= 50 and np.array_equal(whole[0], st[0]["beta"])
    assert not first[3], first[1:]
    assert np.max(np.abs(JS.problem("late_rows_300")[1]["cholesky"][300][:, 256:])) > 0.1  # the late rows reach the weights


@pytest.mark.parametrize("name", JS.MASKED)
def test_masked_statement_converges_from_zero(name):
    held = JS.mask(name)
    st = JS.masked_reference(name)
    assert 0.15 < held.mean() < 0.25
    assert all(s["converged"] and s["decrement"] <= NEWTON_TOL for s in st)
