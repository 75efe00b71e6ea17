"""Co-smoothing, host side: channel folds, the C ABI declares, binds and exports vlgp_replicate_groups at ABI 3, the
co-smoothing score and the argmax rule of cross_validate, and model_selection stays clear of the oracle."""
import ast
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vlgp_hip.h")


@pytest.mark.parametrize("n_ch, n_folds", [(14, 5), (100, 5), (100, 10), (7, 7), (12, 1), (70, 3)])
def test_channel_folds_partition_evenly(n_ch, n_folds):
    from vlgp_amd.evaluation import channel_folds

    folds = channel_folds(n_ch, n_folds, seed=3)
    assert len(folds) == n_folds
    assert all(f == sorted(f) and all(isinstance(c, int) for c in f) for f in folds)
    assert sorted(c for f in folds for c in f) == list(range(n_ch))
    sizes = [len(f) for f in folds]
    assert max(sizes) - min(sizes) <= 1 and min(sizes) >= 1


def test_channel_folds_are_a_function_of_their_arguments():
    from vlgp_amd.evaluation import channel_folds

    assert channel_folds(40, 5, seed=7) == channel_folds(40, 5, seed=7)
    assert channel_folds(40, 5) == channel_folds(40, 5, seed=0)
    assert channel_folds(40, 5, seed=7) != channel_folds(40, 5, seed=8)
    perm = np.random.default_rng(7).permutation(40)  # the stated construction: the permutation dealt round-robin
    assert channel_folds(40, 5, seed=7) == [sorted(int(c) for c in perm[f::5]) for f in range(5)]


@pytest.mark.parametrize("n_ch, n_folds", [(5, 0), (5, 6), (5, -1), (0, 1)])
def test_channel_folds_refuse_impossible_counts(n_ch, n_folds):
    from vlgp_amd.evaluation import channel_folds

    with pytest.raises(ValueError):
        channel_folds(n_ch, n_folds)


def test_header_declares_and_binding_binds_replicate_groups():
    from vlgp_amd import _lib

    text = open(HEADER).read()
    proto = ("int vlgp_replicate_groups(vlgp_ctx* ctx, int src, int dst, int n_rep, const int* group_start, "
             "const int* channel);")
    assert proto in text
    # appended: the new prototype follows every other one
    last = [m.start() for m in re.finditer(r"^int vlgp_[a-z_0-9]+\(", text, flags=re.M)][-1]
    assert text.index(proto) == last
    assert int(re.search(r"#define VLGP_ABI_VERSION (\d+)", text).group(1)) == 3
    assert _lib.ABI_VERSION == 3
    assert "vlgp_replicate_groups" in _lib.EXPORTS
    res, args = _lib._SIGNATURES["vlgp_replicate_groups"]
    assert len(args) == 6


def test_built_library_exports_replicate_groups():
    from vlgp_amd import _lib

    # (as tests/test_host_logic.py checks the header's symbols: through the loaded library.  load() itself raises
    # ImportError when the symbol is missing, so a stale build fails here at the call, not at the assertion)
    lib = _lib.load()
    assert hasattr(lib, "vlgp_replicate_groups"), "libvlgp_hip.so lacks vlgp_replicate_groups"
    assert lib.vlgp_abi_version() == 3


def test_stale_library_is_an_import_error_that_names_the_symbol(monkeypatch):
    from vlgp_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "_SIGNATURES", dict(_lib._SIGNATURES, vlgp_not_in_this_build=(None, [])))
    with pytest.raises(ImportError, match="vlgp_not_in_this_build"):
        _lib.load()


def test_co_bits_per_spike_formula_and_nan_rule():
    from vlgp_amd.evaluation import co_bits_per_spike

    ll = np.array([-10.0, -20.0, -5.0, -7.0])
    ll_null = np.array([-12.0, np.nan, -9.0, -7.5])  # channel 1 Gaussian
    ny = np.array([30.0, 11.0, 0.0, 8.0])            # channel 2 silent
    want = ((-10.0 - 7.0) - (-12.0 - 7.5)) / (38.0 * np.log(2.0))
    assert co_bits_per_spike(ll, ll_null, ny) == pytest.approx(want, rel=1e-15)
    assert np.isnan(co_bits_per_spike(ll[1:3], ll_null[1:3], ny[1:3]))


def test_group_checks_of_leave_group_out_run_before_any_device_work():
    from vlgp_amd.evaluation import _check_groups

    assert _check_groups([[3, 1], (2,)], 5) == [[3, 1], [2]]
    for bad in ([], [[]], [[0], []], [[0, 0]], [[0, 1], [1, 2]], [[5]], [[-1]], [[0, 1, 2, 3, 4]]):
        with pytest.raises(ValueError):
            _check_groups(bad, 5)


def test_best_candidate_rule():
    from vlgp_amd.model_selection import best_candidate

    nan = float("nan")
    assert best_candidate([1, 2, 3], [0.1, 0.3, 0.2]) == 2
    assert best_candidate([3, 1, 2], [0.5, 0.5, 0.4]) == 1   # a tie: the smallest n_factors
    assert best_candidate([1, 2], [nan, -0.4]) == 2          # NaN never wins
    assert best_candidate([1, 2], [nan, nan]) is None


def test_trial_folds_are_contiguous_blocks_of_a_seeded_permutation():
    from vlgp_amd.model_selection import trial_folds

    folds = trial_folds(10, 4, seed=5)
    perm = [int(i) for i in np.random.default_rng(5).permutation(10)]
    assert [i for f in folds for i in f] == perm
    assert [len(f) for f in folds] == [3, 3, 2, 2]
    with pytest.raises(ValueError):
        trial_folds(3, 4)


def test_cross_validate_takes_no_comm():
    from vlgp_amd.model_selection import cross_validate

    with pytest.raises(ValueError, match="comm"):
        cross_validate([{"y": np.zeros((10, 4))}] * 4, [1], comm=None)


def test_model_selection_is_exported_and_never_imports_the_oracle():
    import vlgp_amd

    assert vlgp_amd.model_selection.cross_validate is vlgp_amd.cross_validate
    tree = ast.parse(open(os.path.join(ROOT, "vlgp_amd", "model_selection.py")).read())
    names = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names += [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            names.append(node.module or "")
    assert names and not any("oracle" in n for n in names), names
