"""Generate tests/golden/joint_hstep.npz from the REAL reference: ``gp.elbo(params, mask, t, mu, post_cov)`` with
``mask = [0, 1, 0]`` on three segments with random symmetric positive definite ``post_cov``, at windows of 8 and 50.

    python tests/golden/gen_joint_hstep.py PATH_TO_THE_REFERENCE_CHECKOUT

Not run by the tests.  The output is data only: the seeded inputs and the ``ll`` and ``dll`` the reference returned."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = {  # name: (window, (sigma^2, omega, gp_noise), dt, seed)
    "w8": (8, (1.0, 2e-2, 1e-4), 1.0, 1),
    "w50": (50, (0.7, 3e-3, 1e-4), 1.0, 2),
}
SEGMENTS = 3


def post_cov_of(A):
    """post_cov (W, W, SEGMENTS) = A_i A_i' + 0.05 I from A (W, q, SEGMENTS): symmetric positive definite.  The fixture
    stores A, which keeps it at a few KB; tests/test_joint_hstep_host.py rebuilds post_cov with this very expression."""
    W = A.shape[0]
    return np.stack([A[:, :, i] @ A[:, :, i].T + 0.05 * np.eye(W) for i in range(A.shape[2])], axis=2)


def inputs(W, seed):
    """mu (W, SEGMENTS) and the factors A (W, 3, SEGMENTS) of post_cov."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((W, SEGMENTS)), rng.standard_normal((W, 3, SEGMENTS)) / np.sqrt(3.0)


def main(reference):
    sys.path.insert(0, reference)
    import vlgp.gp as gp

    out = {}
    for name, (W, hyper, dt, seed) in CASES.items():
        mu, A = inputs(W, seed)
        t = np.arange(W) * dt
        ll, dll = gp.elbo(np.array(hyper), np.array([0, 1, 0]), t, mu, post_cov_of(A))
        out.update({name + "_hyper": np.array(hyper), name + "_dt": np.array(dt), name + "_mu": mu, name + "_A": A,
                    name + "_ll": np.array(ll), name + "_dll": np.array(dll)})
    np.savez_compressed(os.path.join(HERE, "joint_hstep.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
