"""NumPy statements of the support kernels (csrc/misc.hip, csrc/sample.hip) that tests/test_gpu_support_shapes.py compares
the device with; the prior factor's statement is the oracle's ichol_gauss.  Every function takes the number type it
computes in, so that tests/test_support_shapes_host.py can show a float64 result equal to the np.longdouble one."""
import numpy as np

U = 2.0 ** -53  # unit roundoff of float64


def project(y, proj, shift, dtype=np.float64):
    """(mu, column sums of y): mu = y proj - shift  (preprocess.initialize's device half, launch_project)."""
    y, proj, shift = (np.asarray(a, dtype=dtype) for a in (y, proj, shift))
    return y @ proj - shift[None, :], y.sum(axis=0)


def project_bound(y, proj, shift):
    """|err| <= (K + 2) u S per element of mu: K = N products, S = sum_n |y_n p_nl| + |shift_l| -- any order, fma or not."""
    S = np.abs(y).astype(np.longdouble) @ np.abs(proj).astype(np.longdouble) + np.abs(shift).astype(np.longdouble)[None, :]
    return (y.shape[1] + 2) * U * S


def latent_map(mu, mat, shift=None, dtype=np.float64):
    """(mu - shift) mat, row by row  (constrain_latent / constrain_loading, launch_latent_map)."""
    mu, mat = np.asarray(mu, dtype=dtype), np.asarray(mat, dtype=dtype)
    if shift is not None:
        mu = mu - np.asarray(shift, dtype=dtype)[None, :]
    return mu @ mat


def latent_map_bound(mu, mat, shift=None):
    """(K + 2) u S per element: K = L products, S = sum_l (|mu_l| + |shift_l|) |m_lc| (the subtraction rounds once)."""
    m = np.abs(mu).astype(np.longdouble)
    if shift is not None:
        m = m + np.abs(shift).astype(np.longdouble)[None, :]
    return (mu.shape[1] + 2) * U * (m @ np.abs(mat).astype(np.longdouble))


def cut(arr, starts, window):
    """Rows [s, s + window) of arr for every start, one after the other  (launch_gather)."""
    return np.concatenate([arr[int(s):int(s) + window] for s in starts], axis=0)


def merge(parent, segs, starts, window):
    """A copy of parent with segment k assigned to its rows [s_k, s_k + window), in order: the later unit wins  (launch_scatter)."""
    out = parent.copy()
    for k, s in enumerate(starts):
        out[int(s):int(s) + window] = segs[k * window:(k + 1) * window]
    return out


def factor_rank(G):
    """Leading columns up to the last non-zero one, at least 1  (prior_rank_kernel, the first pass of sample_posterior_kernel)."""
    nz = np.flatnonzero(np.any(G != 0.0, axis=0))
    return int(nz[-1]) + 1 if nz.size else 1


def sample_posterior(mu, w, G, eps, dtype=np.longdouble):
    """mu_l + G_l Lc^-T eps_l with Lc Lc' = I + G_l' W_l G_l, r_l = factor_rank(G_l) leading columns: plain loops in `dtype`, no
    LAPACK.  mu, w (T, L); G (L, T, R); eps (L, R, n), rows past r_l not read.  Returns (n, T, L)."""
    mu, w, G, eps = (np.asarray(a, dtype=dtype) for a in (mu, w, G, eps))
    T, L = mu.shape
    n = eps.shape[2]
    out = np.empty((n, T, L), dtype=dtype)
    for l in range(L):
        r = factor_rank(G[l])
        Gl = G[l][:, :r]
        H = np.eye(r, dtype=dtype)
        for i in range(r):
            for j in range(i + 1):
                H[i, j] = H[i, j] + np.sum(w[:, l] * Gl[:, i] * Gl[:, j])
        C = np.zeros((r, r), dtype=dtype)
        for k in range(r):
            C[k, k] = np.sqrt(H[k, k] - np.sum(C[k, :k] * C[k, :k]))
            for i in range(k + 1, r):
                C[i, k] = (H[i, k] - np.sum(C[i, :k] * C[k, :k])) / C[k, k]
        z = np.zeros((r, n), dtype=dtype)
        for i in range(r - 1, -1, -1):
            acc = eps[l, i].copy()
            for j in range(i + 1, r):
                acc = acc - C[j, i] * z[j]
            z[i] = acc / C[i, i]
        draw = np.zeros((T, n), dtype=dtype)
        for c in range(r):
            draw = draw + Gl[:, [c]] * z[[c], :]
        out[:, :, l] = (mu[:, [l]] + draw).T
    return out


def draw_bound_w0(mu, G, eps):
    """w == 0: H = I, a draw is mu + G eps.  (K + 2) u S per element, K = r_l products, S = |mu| + sum_c |G_tc eps_cs|."""
    T, L = mu.shape
    n = eps.shape[2]
    out = np.empty((n, T, L), dtype=np.longdouble)
    for l in range(L):
        r = factor_rank(G[l])
        S = np.abs(G[l][:, :r]).astype(np.longdouble) @ np.abs(eps[l, :r]).astype(np.longdouble) + np.abs(mu[:, [l]])
        out[:, :, l] = ((r + 2) * U * S).T
    return out
