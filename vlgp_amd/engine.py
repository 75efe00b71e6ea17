"""Host side of the MI355X vEM engine.

Two layers:

* :class:`Engine` -- one opaque handle of ``libvlgp_hip.so`` per GPU; NumPy in,
  NumPy out, every heavy operation is a HIP kernel behind the C ABI.
* the reference's inner seam, with the reference's names, argument meaning
  and in-place mutation semantics (vlgp/core.py, vlgp/gp.py)::

      estep | mstep | hstep | update_w | update_v | make_cholesky | infer
      | constrain_loading | constrain_latent | vem   (trials, params, config) -> None

  Called on plain lists of trial dicts they upload, run and download (that is
  what the stage-wise parity tests do); called on a :class:`DeviceTrials` --
  what :func:`vlgp_amd.fit` builds -- the data stays resident on the GPU and
  nothing crosses PCIe between stages.
"""
import collections
import ctypes as C
import logging
import os
import time

import numpy as np

from . import _lib
from ._lib import VlgpError, check, dptr, i64ptr, iptr, u8ptr

logger = logging.getLogger(__name__)

__all__ = ["Engine", "DeviceTrials", "estep", "mstep", "hstep", "update_w", "update_v",
           "make_cholesky", "infer", "vem", "constrain_loading", "constrain_latent", "VlgpError"]


# which kernel family ran the most recent seam call on a temporary engine (the engine is gone by the time the
# caller could ask it): "estep" / "update_w" / "update_v" -> one of _lib.ESTEP_PATHS.  Read by the parity tests.
TRACE = {}


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _all_ones(x):
    """x == 1 everywhere; O(1) for the zero-stride view preprocess.initialize hands out."""
    x = np.asarray(x)
    if x.size and all(st == 0 for st in x.strides):
        return bool(x.flat[0] == 1.0)
    return bool(np.all(x == 1.0))


def pack_mask(mask):
    """Bool array (..., N) -> uint64 words (..., (N + 63) // 64), bit ``n & 63`` of word ``n >> 6`` for channel ``n``: the
    layout of vlgp_replicate_masked."""
    mask = np.asarray(mask, dtype=bool)
    N = mask.shape[-1]
    nw = (N + 63) // 64
    padded = np.zeros(mask.shape[:-1] + (nw * 64,), dtype=np.uint8)
    padded[..., :N] = mask
    by = np.packbits(padded, axis=-1, bitorder="little")  # byte j holds channels 8 j ... 8 j + 7, low bit first
    return np.ascontiguousarray(by).view("<u8").reshape(mask.shape[:-1] + (nw,)).astype(np.uint64, copy=False)


def unpack_mask(words, n_channels):
    """The inverse of ``pack_mask``: uint64 words (..., nw) -> bool (..., n_channels)."""
    words = np.ascontiguousarray(words, dtype="<u8")
    bits = np.unpackbits(words.view(np.uint8), axis=-1, bitorder="little")
    return bits[..., :int(n_channels)].astype(bool)


def pack_cov(cov, rows, n_latents):
    """Per-row covariances as vlgp_predictive_cov takes them: float64 (rows, L (L + 1) / 2), the pair ``(l, l')``,
    ``l' <= l``, at ``l (l + 1) / 2 + l'``.  ``cov``: that packed form, or (rows, L, L), of which the lower triangle is
    read."""
    L = int(n_latents)
    cov = np.asarray(cov, dtype=float)
    il, jl = np.tril_indices(L)  # (row-major over the lower triangle: exactly the packed order)
    if cov.shape == (rows, L, L):
        cov = cov[:, il, jl]
    if cov.shape != (rows, len(il)):
        raise ValueError("cov must be (%d, %d, %d) or packed (%d, %d), got %r" % (rows, L, L, rows, len(il), cov.shape))
    return _f64(cov)


def unpack_cov(packed, n_latents):
    """The inverse of ``pack_cov``: (rows, L (L + 1) / 2) -> symmetric (rows, L, L)."""
    L = int(n_latents)
    il, jl = np.tril_indices(L)
    out = np.empty((packed.shape[0], L, L))
    out[:, il, jl] = packed
    out[:, jl, il] = packed
    return out


MAX_NODES = 64  # the largest quadrature rule vlgp_predictive takes


def hermite_nodes(n):
    """Node tables of the ``n``-point Gauss-Hermite rule as vlgp_predictive takes them, ``1 <= n <= 64``:
    ``(z, lwa)`` with ``z = sqrt(2) x`` and ``lwa = log(w / sqrt(pi)) + x ** 2`` for
    ``(x, w) = numpy.polynomial.hermite.hermgauss(n)`` -- the rule for a standard normal, with the weight of the normal
    whose nodes these are divided out again (``evaluation``'s docstring has the sum they enter)."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= MAX_NODES:
        raise ValueError("n_nodes must be an integer in [1, %d], got %r" % (MAX_NODES, n))
    x, w = np.polynomial.hermite.hermgauss(int(n))
    return _f64(np.sqrt(2.0) * x), _f64(np.log(w / np.sqrt(np.pi)) + x * x)


MAX_BINS, MAX_LEVELS, MAX_COUNT = 32, 4, 65536  # the limits of vlgp_calibration


def check_calibration_args(n_bins, levels, max_count):
    """``(n_bins, levels, max_count)`` as vlgp_calibration takes them -- two ints and a float64 array -- or ValueError:
    ``1 <= n_bins <= 32``, at most 4 levels, every one in (0, 1), ``1 <= max_count <= 65536``."""
    for name, val, top in (("n_bins", n_bins, MAX_BINS), ("max_count", max_count, MAX_COUNT)):
        if isinstance(val, bool) or not isinstance(val, (int, np.integer)) or not 1 <= val <= top:
            raise ValueError("%s must be an integer in [1, %d], got %r" % (name, top, val))
    lev = _f64(np.asarray(levels, dtype=float).reshape(-1) if np.ndim(levels) <= 1 else levels)
    if lev.ndim != 1 or len(lev) > MAX_LEVELS:
        raise ValueError("levels must be a list of at most %d numbers, got %r" % (MAX_LEVELS, levels))
    if not np.all((lev > 0.0) & (lev < 1.0)):
        raise ValueError("every level must lie in (0, 1), got %r" % (levels,))
    return int(n_bins), lev, int(max_count)


class Replicas(collections.namedtuple("Replicas", "n channels by_entry")):
    """What ``Engine.replicate`` made of a set: ``n`` replicas; ``channels``, the left-out channel of every (replica,
    channel) pair in the caller's order, or None when the replicas leave single entries out (``by_entry``)."""


class Engine:
    """One GPU, one handle (include/vlgp_hip.h)."""

    def __init__(self, n_channels, n_latents, xdim, rank, gauss_mask=None, device=0):
        self._hbuf = None
        self.lib = _lib.load()
        self.N, self.L, self.P, self.R = int(n_channels), int(n_latents), int(xdim), int(rank)
        mask = np.zeros(self.N, dtype=np.uint8) if gauss_mask is None else \
            np.ascontiguousarray(np.asarray(gauss_mask, dtype=bool).astype(np.uint8))
        if mask.shape != (self.N,):
            raise ValueError("gauss_mask must have one entry per channel")
        self.gauss = mask.astype(bool)
        h = C.c_void_p()
        rc = self.lib.vlgp_create(int(device), self.N, self.L, self.P, self.R, u8ptr(mask), C.byref(h))
        if rc != 0:
            check(rc, None)
        self.h = h
        self.sets = {}  # set id -> (M, rows, offsets)
        self.replicas = {}  # replicated set id -> Replicas (Engine.replicate)
        self.state_epoch = 0  # bumped by every call that can change a set's mu (em_iteration's norm cache keys on it)
        self.rank, self.world = 0, 1
        self.host_exchange = False

    @classmethod
    def for_params(cls, params, device=0):
        """The handle a params dict describes: its ydim, zdim, xdim, rank and the Gaussian channels of ``likelihood``."""
        return cls(params["ydim"], params["zdim"], params["xdim"], params["rank"],
                   np.asarray(params["likelihood"]) == "gaussian", device=device)

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.vlgp_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        check(rc, self.h)

    def check(self, rc):
        """Raise VlgpError with the handle's message for a non-zero status returned outside this class."""
        check(rc, self.h)

    @property
    def handle_address(self):
        """The vlgp_ctx* as an integer (for native callers of the C ABI: vlgp_amd._lockstep)."""
        return int(self.h.value)

    @property
    def hstep_objective_address(self):
        """Address of vlgp_hstep_objective in the loaded library."""
        return int(C.cast(self.lib.vlgp_hstep_objective, C.c_void_p).value)

    def synchronize(self, main_only=False):
        """Wait for the device: everything, or (main_only) the main stream without a pending M-step lane."""
        self._ck(self.lib.vlgp_synchronize_main(self.h) if main_only else self.lib.vlgp_synchronize(self.h))

    # -- unit sets --------------------------------------------------------
    def upload(self, set_id, trials):
        """Pack a list of trial dicts (keys y, x, mu, v, w) into set ``set_id``."""
        self.state_epoch += 1
        lengths = np.array([tr["y"].shape[0] for tr in trials], dtype=np.int64)
        off = np.zeros(len(trials) + 1, dtype=np.int64)
        np.cumsum(lengths, out=off[1:])
        y = _f64(np.concatenate([tr["y"] for tr in trials], axis=0))
        if y.shape[1] != self.N:
            raise ValueError("trial y has %d channels, engine was built for %d" % (y.shape[1], self.N))
        x = None
        if any(tr.get("x") is not None for tr in trials):
            given = [tr.get("x") for tr in trials]
            for tr, xi in zip(trials, given):
                if xi is not None and tuple(xi.shape) != (tr["y"].shape[0], self.P, self.N):
                    raise ValueError("trial x must be (T, %d, %d)" % (self.P, self.N))
            # the default regressors of preprocess.initialize are x == 1: detected per trial, never packed
            if not (self.P == 1 and all(xi is None or _all_ones(xi) for xi in given)):
                xs = [xi if xi is not None else np.ones((tr["y"].shape[0], self.P, self.N))
                      for tr, xi in zip(trials, given)]
                x = _f64(np.concatenate(xs, axis=0))
        elif self.P != 1:
            raise ValueError("trials without x need xdim == 1")

        def cat(key):
            if any(tr.get(key) is None for tr in trials):
                return None
            arr = _f64(np.concatenate([tr[key] for tr in trials], axis=0))
            if arr.shape != (y.shape[0], self.L):
                raise ValueError("trial %s must be (T, %d)" % (key, self.L))
            return arr

        mu, v, w = cat("mu"), cat("v"), cat("w")
        self._ck(self.lib.vlgp_upload_units(self.h, set_id, len(trials), i64ptr(off), dptr(y), dptr(x),
                                            dptr(mu), dptr(v), dptr(w)))
        self.sets[set_id] = (len(trials), int(off[-1]), off)
        self.replicas.pop(set_id, None)

    def cut(self, src, dst, starts, window):
        self.state_epoch += 1
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        self._ck(self.lib.vlgp_cut_units(self.h, src, dst, len(starts), i64ptr(starts), int(window)))
        off = np.arange(len(starts) + 1, dtype=np.int64) * int(window)
        self.sets[dst] = (len(starts), int(off[-1]), off)
        self.replicas.pop(dst, None)

    def set_overlaps(self, set_id, stage_start, links, link_start):
        """Overlapping units of a copied cut: see vlgp_set_overlaps (include/vlgp_hip.h)."""
        stage_start = np.ascontiguousarray(stage_start, dtype=np.int32)
        links = np.ascontiguousarray(links, dtype=np.int32).reshape(-1, 3)
        link_start = np.ascontiguousarray(link_start, dtype=np.int32)
        self._ck(self.lib.vlgp_set_overlaps(self.h, set_id, len(stage_start) - 1, iptr(stage_start), len(links),
                                            iptr(links), iptr(link_start)))

    def unshare_mu(self, set_id):
        self._ck(self.lib.vlgp_unshare_mu(self.h, set_id))

    def merge(self, cut_set):
        self.state_epoch += 1
        self._ck(self.lib.vlgp_merge_units(self.h, cut_set))

    def download(self, set_id, keys=("mu", "v", "w", "dmu")):
        """dict key -> (rows, L) array for the requested keys."""
        _, rows, _ = self.sets[set_id]
        out = {k: np.empty((rows, self.L)) for k in keys}
        self._ck(self.lib.vlgp_download_units(self.h, set_id, dptr(out.get("mu")), dptr(out.get("v")),
                                              dptr(out.get("w")), dptr(out.get("dmu"))))
        return out

    def stash_mu(self, set_id, restore=False):
        """Keep (or write back) a device-side copy of the set's mu (see vlgp_stash_mu)."""
        self.state_epoch += 1
        self._ck(self.lib.vlgp_stash_mu(self.h, int(set_id), int(bool(restore))))

    def free_units(self, set_id):
        self.state_epoch += 1
        self._ck(self.lib.vlgp_free_units(self.h, set_id))
        self.sets.pop(set_id, None)
        self.replicas.pop(set_id, None)

    def replicate(self, src, dst, channels=None, groups=None, held_out=None):
        """Set ``dst`` := replicas of set ``src``, replica-major units, y / x aliased to ``src``
        (vlgp_replicate_groups).  ``groups``: one replica per list of channels, replica k leaving ``groups[k]`` out of
        its E-step; ``loglik`` then scores one slot per (replica, channel) pair, the groups concatenated in order.
        ``channels``: one replica per entry -- the singleton groups ``[[c] for c in channels]``.
        ``held_out``: a bool array (n_rep, rows, N), replica k leaving the single entries ``held_out[k]`` out
        (vlgp_replicate_masked); ``loglik`` then scores one slot per (replica, channel)."""
        if sum(arg is not None for arg in (channels, groups, held_out)) != 1:
            raise ValueError("replicate takes channels, groups or held_out")
        self.state_epoch += 1
        m, rows, off = self.sets[src]
        if held_out is not None:
            held_out = np.asarray(held_out)
            if held_out.dtype != np.bool_ or held_out.ndim != 3 or held_out.shape[1:] != (rows, self.N):
                raise ValueError("held_out must be a bool array (n_rep, %d, %d)" % (rows, self.N))
            k = held_out.shape[0]
            words = pack_mask(held_out)
            self._ck(self.lib.vlgp_replicate_masked(self.h, int(src), int(dst), k,
                                                    words.ctypes.data_as(C.POINTER(C.c_uint64))))
            ch = None
        else:
            if groups is None:
                groups = np.asarray(channels, dtype=np.int32).reshape(-1, 1)
            groups = [np.asarray(g, dtype=np.int32).reshape(-1) for g in groups]
            k = len(groups)
            start = np.zeros(k + 1, dtype=np.int32)
            np.cumsum([len(g) for g in groups], out=start[1:])
            ch = np.ascontiguousarray(np.concatenate(groups) if k else np.zeros(0), dtype=np.int32)
            self._ck(self.lib.vlgp_replicate_groups(self.h, int(src), int(dst), k, iptr(start), iptr(ch)))
        roff = np.concatenate([r * rows + off[:-1] for r in range(k)] + [np.array([k * rows], dtype=np.int64)])
        self.sets[dst] = (k * m, k * rows, roff)
        self.replicas[dst] = Replicas(k, ch, held_out is not None)

    def _score_shapes(self, set_id):
        """``(sums, per-entry)`` shapes of a row score (``loglik``, ``predictive``) of a plain, replicated or masked set."""
        _, rows, _ = self.sets[set_id]
        rep = self.replicas.get(set_id)
        if rep is None:
            return (self.N, 4), (rows, self.N)
        if rep.by_entry:
            return (rep.n, self.N, 4), (rows // max(rep.n, 1), self.N)
        return (len(rep.channels), 4), (rows // max(rep.n, 1), len(rep.channels))

    def _check_eps(self, set_id, eps):
        """The normals of ``marginal`` and ``joint_laplace`` as float64, (units, L, R, n_samples >= 1), and n_samples."""
        units, eps = self.sets[set_id][0], _f64(eps)
        if eps.ndim != 4 or eps.shape[:3] != (units, self.L, self.R) or eps.shape[3] < 1:
            raise ValueError("eps must be (%d, %d, %d, n_samples >= 1), got %r" % (units, self.L, self.R, eps.shape))
        return eps, eps.shape[3]

    def loglik(self, set_id, vb=True, want_rate=False):
        """Plug-in rates and per-channel log-likelihood sums of a set (vlgp_loglik): ``(sums, rate)``, sums
        (slots, 4) and rate (rows, slots) or None; slots = N for a plain set, the (replica, left-out channel) pairs in
        the order of the channel list for a replicated one (rows: the source set's).  A set replicated with
        ``held_out``: sums (n_rep, N, 4) over the entries each replica holds out, rate (rows of the source, N), NaN
        where no replica holds the entry out."""
        sums, entry = self._score_shapes(set_id)
        sums, rate = np.empty(sums), np.empty(entry) if want_rate else None
        self._ck(self.lib.vlgp_loglik(self.h, int(set_id), int(bool(vb)), dptr(rate), dptr(sums)))
        return sums, rate

    def _moments(self, set_id, mu, cov):
        """The ``mu, cov`` of ``predictive`` and ``calibration`` as the ``_cov`` entry points take them: None, None, or
        float64 ``mu`` (rows of the set, L) and ``cov`` packed (rows, L (L + 1) / 2) from either form (``pack_cov``)."""
        if mu is None and cov is None:
            return None, None
        if mu is None or cov is None:
            raise ValueError("mu and cov go together: a posterior mean and covariance per row of the set")
        rows = self.sets[set_id][1]
        mu = _f64(mu)
        if mu.shape != (rows, self.L):
            raise ValueError("mu must be (%d, %d), got %r" % (rows, self.L, mu.shape))
        return mu, pack_cov(cov, rows, self.L)

    def predictive(self, set_id, n_nodes=12, vb=True, want_rate=False, want_lpd=False, mu=None, cov=None):
        """Posterior-predictive log density of a set's entries (vlgp_predictive): ``(sums, rate, lpd)``.  ``sums`` has
        the shape and slots of ``loglik``'s with ``sum lpd`` in column 0; ``rate`` (``loglik``'s plug-in rate) and
        ``lpd`` have the shape of ``loglik``'s rate, or are None.  ``n_nodes``: points of the mode-centred Gauss-Hermite
        rule of the Poisson channels (``hermite_nodes``).  ``mu`` (rows of the set, L) and ``cov`` (those rows, L, L), or
        packed as ``joint_posterior`` unpacks it: score under this posterior of the latents instead of the set's own
        ``mu, v`` (vlgp_predictive_cov; ``vb`` is then not read).  Changes no state."""
        z, lwa = hermite_nodes(n_nodes)
        mu, cov = self._moments(set_id, mu, cov)
        sums, entry = self._score_shapes(set_id)
        sums, rate, lpd = np.empty(sums), np.empty(entry) if want_rate else None, np.empty(entry) if want_lpd else None
        if mu is not None:
            self._ck(self.lib.vlgp_predictive_cov(self.h, int(set_id), len(z), dptr(z), dptr(lwa), dptr(mu), dptr(cov),
                                                  dptr(rate), dptr(lpd), dptr(sums)))
            return sums, rate, lpd
        self._ck(self.lib.vlgp_predictive(self.h, int(set_id), int(bool(vb)), len(z), dptr(z), dptr(lwa), dptr(rate),
                                          dptr(lpd), dptr(sums)))
        return sums, rate, lpd

    def calibration(self, set_id, n_bins=10, levels=(0.5, 0.9), n_nodes=12, vb=True, max_count=4096, want_cdf=False,
                    mu=None, cov=None):
        """Calibration sums of a set's predictive distribution (vlgp_calibration): ``(sums, cdf)``.  ``sums`` has the
        leading shape of ``predictive``'s sums and ``W = n_bins + len(levels) + 3`` columns per slot,
        ``pit_0 ... | covered_0 ... | pearson | entries | skipped`` (``evaluation.calibration_from_sums`` reads them);
        ``cdf``, with ``want_cdf``, has the per-entry shape of ``predictive``'s ``lpd`` plus ``(2,)``: ``F(y - 1), F(y)``,
        NaN for a skipped entry (a Poisson count that is negative, no integer, not finite or above ``max_count``), else
        None.  ``mu``, ``cov``: as ``predictive`` takes them (vlgp_calibration_cov); an entry whose moments are not finite
        is skipped.  The arguments are checked before any device call.  Changes no state."""
        n_bins, levels, max_count = check_calibration_args(n_bins, levels, max_count)
        z, lwa = hermite_nodes(n_nodes)
        mu, cov = self._moments(set_id, mu, cov)
        sums, entry = self._score_shapes(set_id)
        sums = np.empty(sums[:-1] + (n_bins + len(levels) + 3,))
        cdf = np.empty(entry + (2,)) if want_cdf else None
        if mu is not None:
            self._ck(self.lib.vlgp_calibration_cov(self.h, int(set_id), len(z), dptr(z), dptr(lwa), dptr(mu), dptr(cov),
                                                   n_bins, len(levels), dptr(levels) if len(levels) else None, max_count,
                                                   dptr(cdf), dptr(sums)))
            return sums, cdf
        self._ck(self.lib.vlgp_calibration(self.h, int(set_id), int(bool(vb)), len(z), dptr(z), dptr(lwa), n_bins,
                                           len(levels), dptr(levels) if len(levels) else None, max_count, dptr(cdf),
                                           dptr(sums)))
        return sums, cdf

    def pair_moments(self, set_id, vb=True, mu=None, cov=None):
        """Pair moments of a set's predictive distribution (vlgp_pair_moments): ``(resid, model)``, the sums over the rows
        of the products of residuals ``(y - mean)_n (y - mean)_m`` and of the predictive covariance of the two channels
        (``evaluation``'s docstring has the closed forms).  Both are (N, N) for a plain set and (n_rep, N, N) for a set
        replicated with ``held_out=``, where replica ``k`` adds a row to the pair ``(n, m)`` when it holds both entries out;
        both are symmetric to the bit.  ``mu``, ``cov``: as ``predictive`` takes them (vlgp_pair_moments_cov; ``vb`` is then
        not read); a row whose ``mu`` or ``cov`` holds a non-finite value adds nothing.  Changes no state."""
        mu, cov = self._moments(set_id, mu, cov)
        rep = self.replicas.get(set_id)
        shape = (self.N, self.N) if rep is None else (rep.n, self.N, self.N)
        resid, model = np.empty(shape), np.empty(shape)
        if mu is not None:
            self._ck(self.lib.vlgp_pair_moments_cov(self.h, int(set_id), dptr(mu), dptr(cov), dptr(resid), dptr(model)))
        else:
            self._ck(self.lib.vlgp_pair_moments(self.h, int(set_id), int(bool(vb)), dptr(resid), dptr(model)))
        return resid, model

    def lag_moments(self, set_id, max_lag, vb=True):
        """Lag moments of a set's predictive distribution (vlgp_lag_moments): ``(resid, model, count, n_failed)``, per
        lag ``k = 0 ... max_lag`` and channel the sums over the pairs of rows ``(t, t + k)`` of one unit of the products of
        residuals, of the predictive covariance of the two counts (``evaluation``'s docstring has the closed forms) and
        the number of pairs.  (max_lag + 1, N) each for a plain set, (n_rep, max_lag + 1, N) for a set replicated with
        ``held_out=``, where replica ``k`` counts a pair when it holds both entries out.  ``n_failed``: the (unit, latent)
        pairs whose ``H`` could not be factored; their units add nothing.  Needs bound priors.  Changes no state."""
        max_lag = int(max_lag)
        if max_lag < 0:  # (nothing to size the outputs by; the library refuses a lag past 64)
            raise ValueError("max_lag = %d, need 0 <= max_lag <= 64" % max_lag)
        rep = self.replicas.get(set_id)
        shape = (max_lag + 1, self.N) if rep is None else (rep.n, max_lag + 1, self.N)
        resid, model, count = np.empty(shape), np.empty(shape), np.empty(shape)
        n = C.c_int(0)
        self._ck(self.lib.vlgp_lag_moments(self.h, int(set_id), int(bool(vb)), max_lag, dptr(resid), dptr(model),
                                           dptr(count), C.byref(n)))
        return resid, model, count, n.value

    def elbo(self, set_id, vb=True, want_rows=False):
        """Terms of the variational lower bound of a plain set (vlgp_elbo): ``(row_sums, kl_terms, n_failed, row_ell)``
        -- row_sums (N, 4) per channel, kl_terms (units, L, 4) = log det H, tr H^-1, beta'beta, |mu - G beta|^2 per
        (unit, latent), the number of pairs whose factorisation failed (their terms are NaN), and with ``want_rows``
        the expected log-likelihood of every row summed over the channels (else None).  Changes no state."""
        units, rows, _ = self.sets[set_id]
        sums = np.empty((self.N, 4))
        terms = np.empty((units, self.L, 4))
        row_ell = np.empty(rows) if want_rows else None
        n = C.c_int(0)
        self._ck(self.lib.vlgp_elbo(self.h, int(set_id), int(bool(vb)), dptr(sums), dptr(row_ell), dptr(terms),
                                    C.byref(n)))
        return sums, terms, n.value, row_ell

    def forecast(self, set_id, ext, vb=True):
        """The posterior of a plain set carried past the last row of every unit (vlgp_forecast).  ``ext``:
        ``{length: G_ext (L, n_ext, R)}`` for every unit length of the set, the rows that follow the bound prior factor
        in the same factorisation.  Returns ``(mu_ext, v_ext, fit_terms, n_failed)``: mu_ext, v_ext
        (sum over the units of their n_ext, L), unit-major; fit_terms (units, L, 2) = ``|G beta - mu|^2, |mu|^2``; the
        number of (unit, latent) tasks whose factorisation failed (their outputs are NaN).  Changes no state."""
        units, _, off = self.sets[set_id]
        lengths = np.ascontiguousarray(sorted(int(T) for T in ext), dtype=np.int32)
        blocks = [_f64(ext[int(T)]) for T in lengths]
        for T, G in zip(lengths, blocks):
            if G.ndim != 3 or G.shape[0] != self.L or G.shape[2] != self.R:
                raise ValueError("extension rows for length %d must be (%d, n_ext, %d), got %r"
                                 % (T, self.L, self.R, G.shape))
        n_ext = np.ascontiguousarray([G.shape[1] for G in blocks], dtype=np.int32)
        by_len = dict(zip(lengths.tolist(), n_ext.tolist()))
        total = sum(by_len.get(int(T), 0) for T in np.diff(np.asarray(off)))  # (an unlisted length: the library says so)
        G_all = _f64(np.concatenate([G.ravel() for G in blocks])) if blocks else np.zeros(0)
        mu_ext, v_ext = np.empty((total, self.L)), np.empty((total, self.L))
        terms = np.empty((units, self.L, 2))
        n = C.c_int(0)
        self._ck(self.lib.vlgp_forecast(self.h, int(set_id), int(bool(vb)), len(lengths), iptr(lengths), iptr(n_ext),
                                        dptr(G_all), dptr(mu_ext), dptr(v_ext), dptr(terms), C.byref(n)))
        return mu_ext, v_ext, terms, n.value

    def marginal(self, set_id, eps, vb=True, want_parts=False):
        """Importance weights of ``log p(y_unit)`` for every unit of a plain set under joint draws of its latent paths
        from the fitted posterior (vlgp_marginal).  ``eps``: (units, L, R, n_samples) standard normals, the sample index
        last; rows beyond a (unit, latent)'s effective rank are not read.  Returns ``(log_w, n_failed, parts)``: log_w
        (units, n_samples); the number of (unit, latent) pairs whose factorisation failed (their unit's log_w is NaN);
        with ``want_parts`` (units, n_samples, 2) = the log-likelihood of the draw and the prior-over-proposal term, which
        add to log_w (else None).  Changes no state."""
        units, _, _ = self.sets[set_id]
        eps, K = self._check_eps(set_id, eps)
        log_w = np.empty((units, K))
        parts = np.empty((units, K, 2)) if want_parts else None
        n = C.c_int(0)
        self._ck(self.lib.vlgp_marginal(self.h, int(set_id), int(bool(vb)), K, dptr(eps), dptr(log_w), dptr(parts),
                                        C.byref(n)))
        return log_w, n.value, parts

    def joint_laplace(self, set_id, max_iter=50, tol=1e-10, eps=None):
        """Joint Laplace posterior of every unit of a plain set (vlgp_joint_laplace): the mode of the posterior over all
        prior weights of a unit by a damped Newton iteration started at the mean-field centres of the set's current
        ``mu, w``.  ``eps``: None, or (units, L, R, n_samples) standard normals as ``marginal`` takes them, for draws from
        the joint Gaussian ``N(beta, H^-1)``.  Returns a dict: ``beta`` (units, L, R); ``stats`` (units, 8) and its columns
        ``laplace``, ``ll``, ``beta_sq``, ``logdet``, ``decrement``, ``n_newton``, ``converged``, ``D``; ``mu``, ``v``
        (rows, L); ``n_failed`` (units whose ``H`` could not be factored: their numbers are NaN); with ``eps`` also
        ``log_w`` (units, n_samples) and ``parts`` (units, n_samples, 2) = the log-likelihood of the draw and the
        prior-over-proposal term, which add to ``log_w``.  Changes no state."""
        units, rows, _ = self.sets[set_id]
        K, log_w, parts = 0, None, None
        if eps is not None:
            eps, K = self._check_eps(set_id, eps)
            log_w, parts = np.empty((units, K)), np.empty((units, K, 2))
        beta = np.empty((units, self.L, self.R))
        stats = np.empty((units, 8))
        mu, v = np.empty((rows, self.L)), np.empty((rows, self.L))
        n = C.c_int(0)
        self._ck(self.lib.vlgp_joint_laplace(self.h, int(set_id), int(max_iter), float(tol), K, dptr(eps), dptr(beta),
                                             dptr(stats), dptr(mu), dptr(v), dptr(log_w), dptr(parts), C.byref(n)))
        out = {"beta": beta, "stats": stats, "mu": mu, "v": v, "n_failed": n.value,
               "laplace": stats[:, 0].copy(), "ll": stats[:, 1].copy(), "beta_sq": stats[:, 2].copy(),
               "logdet": stats[:, 3].copy(), "decrement": stats[:, 4].copy(), "n_newton": stats[:, 5].astype(np.int64),
               "converged": stats[:, 6] > 0, "D": stats[:, 7].astype(np.int64)}
        if eps is not None:
            out.update(log_w=log_w, parts=parts)
        return out

    def joint_posterior(self, set_id, max_iter=50, tol=1e-10, window=None):
        """``joint_laplace`` without draws and with the covariance of every row, on a plain set or on a set replicated
        with ``held_out`` of one replica, whose held-out entries the posterior does not see (vlgp_joint_posterior).
        Returns ``joint_laplace``'s dict without ``v``, ``log_w`` and ``parts``, plus ``cov`` (rows, L, L), symmetric:
        ``cov[t, l, l'] = G_l[t] (H^-1)_{l l'} G_l'[t]'``, whose diagonal is ``joint_laplace``'s ``v``.  A failed unit's
        rows of ``mu`` and ``cov`` are NaN.  Changes no state.

        ``window`` (2 ... 64; vlgp_joint_posterior_moments): the same call and the same results, plus
        ``"window_moments"`` (L, window, window), the sum over every window of every unit of
        ``m m' + G_l (H^-1)_ll G_l'`` on the window's rows (``gp.optimize_joint`` takes it; NaN when a unit failed), and
        ``"n_windows"``."""
        units, rows, _ = self.sets[set_id]
        beta = np.empty((units, self.L, self.R))
        stats = np.empty((units, 8))
        mu, packed = np.empty((rows, self.L)), np.empty((rows, self.L * (self.L + 1) // 2))
        n = C.c_int(0)
        extra = {}
        if window is None:
            self._ck(self.lib.vlgp_joint_posterior(self.h, int(set_id), int(max_iter), float(tol), dptr(beta), dptr(stats),
                                                   dptr(mu), dptr(packed), C.byref(n)))
        else:
            w = min(max(int(window), 0), 65)  # (only the size of the buffer: the library refuses what is out of range)
            S, n_w = np.empty((self.L, w, w)), np.zeros(1, dtype=np.int64)
            self._ck(self.lib.vlgp_joint_posterior_moments(self.h, int(set_id), int(max_iter), float(tol), dptr(beta),
                                                           dptr(stats), dptr(mu), dptr(packed), C.byref(n), int(window),
                                                           dptr(S), i64ptr(n_w)))
            extra = {"window_moments": S, "n_windows": int(n_w[0])}
        return dict({"beta": beta, "stats": stats, "mu": mu, "cov": unpack_cov(packed, self.L), "n_failed": n.value,
                     "laplace": stats[:, 0].copy(), "ll": stats[:, 1].copy(), "beta_sq": stats[:, 2].copy(),
                     "logdet": stats[:, 3].copy(), "decrement": stats[:, 4].copy(),
                     "n_newton": stats[:, 5].astype(np.int64), "converged": stats[:, 6] > 0,
                     "D": stats[:, 7].astype(np.int64)}, **extra)

    def unit_ranks(self, set_id):
        """(units, L) effective rank of the prior factor each (unit, latent) of the set is bound to."""
        _, _, off = self.sets[set_id]
        lengths = np.diff(np.asarray(off))
        by_len = {int(T): self.prior_ranks(int(T)) for T in np.unique(lengths)}
        return np.stack([by_len[int(T)] for T in lengths]).astype(np.int64)

    # -- parameters -------------------------------------------------------
    def set_params(self, a, b, noise):
        a, b, noise = _f64(a), _f64(b), _f64(noise)
        if a.shape != (self.L, self.N) or b.shape != (self.P, self.N) or noise.shape != (self.N,):
            raise ValueError("parameter shapes must be a (L,N), b (P,N), noise (N)")
        self._ck(self.lib.vlgp_set_params(self.h, dptr(a), dptr(b), dptr(noise)))

    def set_loading(self, a):
        """Replace the loading matrix only (constrain_loading rescales a and leaves b, noise alone)."""
        a = _f64(a)
        if a.shape != (self.L, self.N):
            raise ValueError("loading matrix must be (L, N)")
        self._ck(self.lib.vlgp_set_params(self.h, dptr(a), None, None))

    def get_params(self):
        a, da = np.empty((self.L, self.N)), np.empty((self.L, self.N))
        b, db = np.empty((self.P, self.N)), np.empty((self.P, self.N))
        noise = np.empty(self.N)
        self._ck(self.lib.vlgp_get_params(self.h, dptr(a), dptr(b), dptr(noise), dptr(da), dptr(db)))
        return a, b, noise, da, db

    # -- prior ------------------------------------------------------------
    def build_prior(self, lengths, omega, sigma):
        lengths = np.ascontiguousarray(np.unique(np.asarray(lengths)) if len(lengths) > 1 else lengths, dtype=np.int32)
        omega, sigma = _f64(omega), _f64(sigma)
        self._ck(self.lib.vlgp_build_prior(self.h, len(lengths), iptr(lengths), dptr(omega), dptr(sigma)))

    def set_prior(self, T, G):
        G = _f64(G)
        if G.shape != (self.L, int(T), self.R):
            raise ValueError("prior factor for length %d must be (%d, %d, %d), got %r"
                             % (T, self.L, T, self.R, G.shape))
        self._ck(self.lib.vlgp_set_prior(self.h, int(T), dptr(G)))

    def clear_prior(self):
        self._ck(self.lib.vlgp_clear_prior(self.h))

    def prior_ranks(self, T):
        """Effective rank (number of columns ichol_gauss built) per latent for length T; no device traffic."""
        rk = np.zeros(self.L, dtype=np.int32)
        self._ck(self.lib.vlgp_get_prior(self.h, int(T), None, iptr(rk)))
        return rk

    def get_prior(self, T, with_rank=False):
        G = np.empty((self.L, int(T), self.R))
        rk = np.zeros(self.L, dtype=np.int32)
        self._ck(self.lib.vlgp_get_prior(self.h, int(T), dptr(G), iptr(rk)))
        return (G, rk) if with_rank else G

    # -- E / M / H --------------------------------------------------------
    def update_w(self, set_id):
        self.state_epoch += 1
        self._ck(self.lib.vlgp_update_w(self.h, set_id))

    def update_v(self, set_id, vb=True, count=True):
        self.state_epoch += 1
        n = C.c_int(0)
        self._ck(self.lib.vlgp_update_v(self.h, set_id, int(bool(vb)), C.byref(n) if count else None))
        return n.value

    def estep(self, set_id, n_iter, dmu_bound=5.0, vb=True, count=True):
        self.state_epoch += 1
        n = C.c_int(0)
        self._ck(self.lib.vlgp_estep(self.h, set_id, int(n_iter), float(dmu_bound), int(bool(vb)),
                                     C.byref(n) if count else None))
        return n.value

    def estep_wait(self):
        """Wait for the most recent estep call's launches (not for work queued behind them since)."""
        self._ck(self.lib.vlgp_estep_wait(self.h))

    def mstep(self, set_id, n_iter, use_hessian=True, eps=1e-8, learning_rate=1.0, da_bound=5.0,
              db_bound=5.0, count=True):
        n = C.c_int(0)
        self._ck(self.lib.vlgp_mstep(self.h, set_id, int(n_iter), int(bool(use_hessian)), float(eps),
                                     float(learning_rate), float(da_bound), float(db_bound),
                                     C.byref(n) if count else None))
        return n.value

    def mstep_cov(self, set_id, mu, cov, n_iter, use_hessian=True, eps=1e-8, learning_rate=1.0, da_bound=5.0,
                  db_bound=5.0):
        """``mstep`` under a full Gaussian posterior per row (vlgp_mstep_cov): ``mu`` (rows of the set, L) and ``cov``
        (those rows, L, L) -- symmetric, checked -- or packed as ``joint_posterior`` unpacks it take the place of the
        set's ``mu, v``, which are not read.  A ``cov`` without off-diagonal entries is ``mstep`` on a set whose ``v`` is
        its diagonal.  Plain sets and cuts, one rank, ``L <= 10``, ``P <= 8``; a non-finite moment is an error that names
        its row and changes no parameter.  Returns the number of channels whose system was not positive definite."""
        return self._mstep_cov(self.lib.vlgp_mstep_cov, set_id, mu, cov, n_iter, use_hessian, eps, learning_rate, da_bound,
                               db_bound)

    def mstep_cov_masked(self, set_id, mu, cov, n_iter, use_hessian=True, eps=1e-8, learning_rate=1.0, da_bound=5.0,
                         db_bound=5.0):
        """``mstep_cov`` of a masked fit set (``replicate(src, dst, held_out=missing[None])``; vlgp_mstep_cov_masked): every
        channel over the rows where it is observed, ``noise`` the variance over those rows; what ``y`` holds at a missing
        entry is not read.  ``mu``, ``cov`` over the rows of the set, as ``joint_posterior`` of that set returns them.  A
        channel without an observed row keeps ``a, b, noise``.  Poisson channels only; a set without a mask is an error
        (``mstep_cov`` takes it).  Arguments, checks and return value as ``mstep_cov``."""
        return self._mstep_cov(self.lib.vlgp_mstep_cov_masked, set_id, mu, cov, n_iter, use_hessian, eps, learning_rate,
                               da_bound, db_bound)

    def _mstep_cov(self, entry, set_id, mu, cov, n_iter, use_hessian, eps, learning_rate, da_bound, db_bound):
        if mu is None or cov is None:
            raise ValueError("mu and cov go together: a posterior mean and covariance per row of the set")
        cov = np.asarray(cov, dtype=float)
        if cov.ndim == 3:  # (the lower triangle is what goes to the device: an asymmetric cov would be silently halved)
            gap = np.abs(cov - cov.transpose(0, 2, 1))
            if np.any(gap > 1e-9 * max(1.0, float(np.nanmax(np.abs(cov), initial=0.0)))):
                raise ValueError("cov must be symmetric in its last two axes")
        mu, cov = self._moments(set_id, mu, cov)
        n = C.c_int(0)
        self._ck(entry(self.h, int(set_id), dptr(mu), dptr(cov), int(n_iter), int(bool(use_hessian)), float(eps),
                       float(learning_rate), float(da_bound), float(db_bound), C.byref(n)))
        return n.value

    def mstep_begin(self, set_id, n_iter, use_hessian=True, eps=1e-8, learning_rate=1.0, da_bound=5.0,
                    db_bound=5.0):
        """Enqueue the M-step on the engine's second stream and return at once."""
        self._ck(self.lib.vlgp_mstep_begin(self.h, set_id, int(n_iter), int(bool(use_hessian)), float(eps),
                                           float(learning_rate), float(da_bound), float(db_bound)))

    def mstep_end(self):
        """Wait for the M-step begun earlier; returns (n_failed, device milliseconds)."""
        n, ms = C.c_int(0), C.c_double(0)
        self._ck(self.lib.vlgp_mstep_end(self.h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def hstep_objective(self, set_id, window, dt, latents, logp, copy=True):
        """Batched (ll, dll) for evaluations (latents[e], logp[e, :3]).  copy=False hands out views of the call's
        persistent result buffers (valid until the next call)."""
        n = len(latents)
        if n > 16:  # a call takes at most 16 evaluations (more than 16 latents in lock-step): in slices
            logp = np.reshape(logp, (n, 3))
            parts = [self.hstep_objective(set_id, window, dt, latents[i:i + 16], logp[i:i + 16]) for i in range(0, n, 16)]
            return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        hb = self._hbuf
        if hb is None or hb[0] < n:  # persistent argument buffers: this is called ~40 times per EM iteration
            cap = max(16, n)
            arrs = (np.zeros(cap, dtype=np.int32), np.zeros((cap, 3)), np.zeros(cap), np.zeros((cap, 3)))
            hb = self._hbuf = (cap, arrs, (iptr(arrs[0]), dptr(arrs[1]), dptr(arrs[2]), dptr(arrs[3])))
        (lat, lp, ll, dll), ptrs = hb[1], hb[2]
        lat[:n] = latents
        lp[:n] = logp if getattr(logp, "shape", None) == (n, 3) else np.reshape(logp, (n, 3))
        self._ck(self.lib.vlgp_hstep_objective(self.h, set_id, int(window), float(dt), n, *ptrs))
        if copy:
            return ll[:n].copy(), dll[:n].copy()
        return ll[:n], dll[:n]

    def project_latent(self, set_id, proj, shift):
        """mu = y @ proj - shift on the device for every row of the set; returns the column sums of y."""
        self.state_epoch += 1
        proj = _f64(proj)
        shift = _f64(shift)
        if proj.shape != (self.N, self.L) or shift.shape != (self.L,):
            raise ValueError("projection must be (N, L) with an (L,) shift")
        colsum = np.empty(self.N)
        self._ck(self.lib.vlgp_project_units(self.h, set_id, dptr(proj), dptr(shift), dptr(colsum)))
        return colsum

    def hstep_prepare(self, set_id, window):
        """Enqueue now what the H-step bracket builds from the units alone (see vlgp_hstep_prepare)."""
        self._ck(self.lib.vlgp_hstep_prepare(self.h, set_id, int(window)))

    def hstep_begin(self, set_id, window):
        """Start of one gp.optimize run: mu, w of the set stay fixed until hstep_end."""
        self._ck(self.lib.vlgp_hstep_begin(self.h, set_id, int(window)))

    def hstep_end(self):
        self._ck(self.lib.vlgp_hstep_end(self.h))

    # -- constraints / norms ----------------------------------------------
    def apply_latent_map(self, set_id, mat, shift=None):
        self.state_epoch += 1
        mat = _f64(mat)
        if mat.shape != (self.L, self.L):
            raise ValueError("latent map must be (L, L)")
        self._ck(self.lib.vlgp_apply_latent_map(self.h, set_id, dptr(mat),
                                                dptr(_f64(shift)) if shift is not None else None))

    def norms(self, set_id):
        out = np.empty(2)
        self._ck(self.lib.vlgp_norms(self.h, set_id, dptr(out)))
        return float(np.sqrt(out[0])), float(np.sqrt(out[1]))

    def norms_begin(self, set_id):
        """Enqueue the norms of mu, dmu (they run beside whatever follows on the main stream); norms_end collects."""
        self._ck(self.lib.vlgp_norms_begin(self.h, set_id))

    def norms_end(self):
        out = np.empty(2)
        self._ck(self.lib.vlgp_norms_end(self.h, dptr(out)))
        return float(np.sqrt(out[0])), float(np.sqrt(out[1]))

    def latent_moments(self, set_id):
        s1, s2 = np.empty(self.L), np.empty(self.L)
        cnt = C.c_double(0)
        self._ck(self.lib.vlgp_latent_moments(self.h, set_id, dptr(s1), dptr(s2), C.byref(cnt)))
        return s1, s2, cnt.value

    # -- multi-GPU --------------------------------------------------------
    def comm_init(self, uid, rank, world, uid_aux=None):
        self._ck(self.lib.vlgp_comm_init(self.h, uid, int(rank), int(world)))
        if uid_aux is not None:
            self._ck(self.lib.vlgp_comm_init_aux(self.h, uid_aux))
        self.rank, self.world = int(rank), int(world)
        self.host_exchange = bool(self.lib.vlgp_comm_host_exchange(self.h))

    @property
    def transport(self):
        """"none" (single rank), "rccl" or "shm" (the opt-in host shared-memory test transport)."""
        return ("none", "rccl", "shm")[int(self.lib.vlgp_comm_transport(self.h))]

    @property
    def rccl_ranks(self):
        """(main lane, M-step lane): the rank counts RCCL reports for the two communicators (ncclCommCount); 0 without."""
        a, b = C.c_int(0), C.c_int(0)
        self._ck(self.lib.vlgp_comm_rccl_ranks(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def allreduce_host(self, arr):
        """In-place sum over ranks of a float64 host array (no-op on one GPU)."""
        if not (isinstance(arr, np.ndarray) and arr.dtype == np.float64 and arr.flags["C_CONTIGUOUS"]):
            raise TypeError("allreduce_host needs a C-contiguous float64 array (the buffer is summed in place as doubles)")
        self._ck(self.lib.vlgp_comm_allreduce_host(self.h, dptr(arr), arr.size))
        return arr

    def barrier(self):
        """Drain this handle's stream and rendezvous with the other ranks."""
        self._ck(self.lib.vlgp_comm_allreduce_host(self.h, None, 0))

    # -- measurement ------------------------------------------------------
    def profile(self, on=True):
        self._ck(self.lib.vlgp_profile_enable(self.h, int(bool(on))))

    def profile_reset(self):
        self._ck(self.lib.vlgp_profile_reset(self.h))

    def phase_clock(self, on=True):
        """Read (and re-arm or disable) the E-step per-phase cycle counters."""
        out = (C.c_uint64 * 8)()
        self._ck(self.lib.vlgp_debug_phase_clock(self.h, int(bool(on)), out))
        return [int(v) for v in out]

    @property
    def last_estep_path(self):
        """Kernel family of the most recent E-step / update_w / update_v: one of _lib.ESTEP_PATHS."""
        p = C.c_int(0)
        self._ck(self.lib.vlgp_debug_last_estep_path(self.h, C.byref(p)))
        return _lib.ESTEP_PATHS[p.value]

    @property
    def last_hstep_path(self):
        """Kernel family of the most recent hstep_objective call: one of _lib.HSTEP_PATHS."""
        p = C.c_int(0)
        self._ck(self.lib.vlgp_debug_last_hstep_path(self.h, C.byref(p)))
        return _lib.HSTEP_PATHS[p.value]

    def reload_switches(self):
        """Read the library's VLGP_* debug switches from the environment again (all are cached at creation)."""
        self._ck(self.lib.vlgp_debug_reload_switches(self.h))

    def switch(self, name):
        """The value this handle holds for the debug switch `name` (flag 0 / 1, tri-state -1 / 0 / 1, integer or real)."""
        v = C.c_double(0)
        self._ck(self.lib.vlgp_debug_switch(self.h, name.encode(), C.byref(v)))
        return v.value

    def hstep_stats(self):
        """(low-rank evaluations, sum of their predicted ranks, dense evaluations, low-rank rounds re-run densely)."""
        out = np.zeros(4)
        self._ck(self.lib.vlgp_debug_hstep_stats(self.h, dptr(out)))
        return out

    def hstep_plan(self):
        """What the most recent ``hstep_objective`` call launched (vlgp_debug_hstep_plan: noted by the launcher where it
        decides, nothing recomputed).  A dict: ``path`` (one of _lib.HSTEP_PATHS), ``rerun`` (the dense round after a
        low-rank overflow); round kernels: TC, nb, wlm; low-rank and mixed rounds also n_lr, n_rough, rmax, rc (the
        register class 16 / 24 / 28 / 32), tabg, fused, lds (doubles), rcap (16 slots, per evaluation); generic kernels:
        nw, tm_global, huge."""
        out = np.zeros(_lib.HSTEP_PLAN_LEN, dtype=np.int32)
        self._ck(self.lib.vlgp_debug_hstep_plan(self.h, iptr(out)))
        o = [int(v) for v in out]
        at = lambda name: o[_lib.HP[name]]
        return dict(path=_lib.HSTEP_PATHS[at("PATH")], rerun=at("RERUN"), TC=at("TC"), nb=at("NB"), wlm=at("WLM"),
                    n_lr=at("N_LR"), n_rough=at("N_ROUGH"), rmax=at("RMAX"), rc=at("CLASS"), tabg=at("TABG"), fused=at("FUSED"),
                    lds=at("LDS"), rcap=o[_lib.HP["RCAP"]:_lib.HP["RCAP"] + 16], nw=at("NW"), tm_global=at("TM_GLOBAL"),
                    huge=at("HUGE"))

    MSTEP_PLAN_KEYS = ("G", "rows_per_wg", "CT", "S", "nthr", "tiles", "LT", "PT", "exact", "fixed", "anyg", "noise_passes")

    def mstep_plan(self, rows):
        """What ``mstep`` would launch for a set of ``rows`` rows on this handle (vlgp_debug_mstep_plan): a dict of the
        geometry (G, rows_per_wg, CT, S, nthr, tiles), the compiled sizes LT, PT (0, 0: the loop-based kernels), whether
        the Newton launch of a set with x == 1 is the EXACT instantiation, FIXED and ANYG of the sum + solve launch, and
        whether the noise takes two passes.  Launches nothing."""
        out = np.zeros(12, dtype=np.int32)
        self._ck(self.lib.vlgp_debug_mstep_plan(self.h, C.c_int64(int(rows)), iptr(out)))
        return dict(zip(self.MSTEP_PLAN_KEYS, (int(v) for v in out)))

    ESTEP_MODES = {"estep": 1 | 2 | 4, "update_w": 4, "update_v": 1 | 8}  # EM_FACTOR0 | EM_MEAN | EM_W | EM_V (csrc/ctx.h)
    ESPLIT_DECLINES = ("taken", "VLGP_ESTEP_SPLIT=0", "VLGP_ESTEP_GENERIC", "L > 10", "N > 1024", "VLGP_ESTEP_LSPLIT=0",
                       "long rank", "long: few tasks", "small set", "rank > 32", "records")  # in the order of _lib.ESPLIT
    ECLASSES = tuple(k.lower() for k in _lib.ECLASS)

    def estep_plan(self, set_id, n_iter, what="estep", vb=True):
        """What ``estep`` / ``update_w`` / ``update_v`` would launch for the resident set (vlgp_debug_estep_plan: the
        dispatch itself, reporting instead of launching).  A dict: ``family`` (one of _lib.ESTEP_PATHS), ``decline`` (why
        the split E-step did not take the set, one of ESPLIT_DECLINES); for the split families LT, REC, maxra, use_lane,
        mix, maxra_hi, rtop, lo_shared_g, n_lanes, cuts, CS, NJ, ranks and classes per latent; fast: LT, RP, RA; generic:
        LT, small, rg."""
        mode = self.ESTEP_MODES[what] | (8 if what == "estep" and vb else 0)
        out = np.zeros(_lib.ESTEP_PLAN_LEN, dtype=np.int32)
        self._ck(self.lib.vlgp_debug_estep_plan(self.h, int(set_id), mode, int(n_iter), iptr(out)))
        o = [int(v) for v in out]
        at = lambda name: o[_lib.EP[name]]
        per_latent = lambda name: o[_lib.EP[name]:_lib.EP[name] + min(self.L, 16)]
        family = _lib.ESTEP_PATHS[at("FAMILY")]
        plan = {"family": family, "decline": self.ESPLIT_DECLINES[at("DECLINE")]}
        if family in ("split", "split_mixed", "long_split"):
            nl = at("N_LANES")
            plan.update(LT=at("LT"), REC=at("REC"), maxra=at("MAXRA"), use_lane=at("USE_LANE"), mix=at("MIX"),
                        maxra_hi=at("MAXRA_HI"), rtop=at("RTOP"), lo_shared_g=at("LO_SHG"), n_lanes=nl,
                        cuts=o[_lib.EP["CUT"]:_lib.EP["CUT"] + nl + 1], CS=at("CS"), NJ=at("NJ"), ranks=per_latent("RANK"),
                        classes=[self.ECLASSES[k] for k in per_latent("CLASS")])
        elif family == "fast":
            plan.update(LT=at("LT"), RP=at("RP"), RA=at("RA"))
        elif family == "generic":
            plan.update(LT=at("LT"), small=at("SMALL"), rg=at("RG"))
        return plan

    def profile_get(self, kind):
        n, ms, units = C.c_int64(0), C.c_double(0), C.c_double(0)
        self._ck(self.lib.vlgp_profile_get(self.h, int(kind), C.byref(n), C.byref(ms), C.byref(units)))
        return n.value, ms.value, units.value


def unique_id():
    """RCCL unique id (rank 0 creates it, every rank passes it to Engine.comm_init)."""
    buf = C.create_string_buffer(_lib.UNIQUE_ID_BYTES)
    check(_lib.load().vlgp_comm_unique_id(buf), None)
    return buf.raw


# ===========================================================================
# the reference's (trials, params, config) seam
# ===========================================================================
class DeviceTrials(list):
    """A list of trial dicts whose arrays are resident on an :class:`Engine`.

    Behaves as the plain list the reference passes around; the host copies of
    mu/v/w/dmu are refreshed only by :meth:`pull` (callbacks, end of fit).
    """

    def __init__(self, trials, engine, set_id, parent_set=None, unit_of=None):
        super().__init__(trials)
        self.engine = engine
        self.set_id = set_id
        self.parent_set = parent_set  # segments: the set of the trials they were cut from
        self.detached = False         # True once the segments' mu stopped writing through (constrain_loading "svd")
        self.unit_of = unit_of        # overlapping segments are stored stage-major: list index -> unit of the set

    def pull(self, keys=("mu", "v", "w", "dmu")):
        """Copy device state into the dicts: mu, v, dmu in place, w rebound
        (exactly the ownership the reference leaves behind, core.py:117-120)."""
        got = self.engine.download(self.set_id, keys)
        _, _, off = self.engine.sets[self.set_id]
        for i, tr in enumerate(self):
            u = i if self.unit_of is None else int(self.unit_of[i])
            sl = slice(int(off[u]), int(off[u + 1]))
            for k in keys:
                if k == "w" or tr.get(k) is None or tr[k].shape != got[k][sl].shape:
                    tr[k] = got[k][sl].copy()
                else:
                    tr[k][...] = got[k][sl]


def _push_params(eng, params):
    eng.set_params(params["a"], params["b"], params["noise"])


def _pull_params(eng, params):
    a, b, noise, da, db = eng.get_params()
    params["a"][...] = a          # in place, like core.py:202,220
    params["b"][...] = b
    params["noise"] = noise       # rebound, like core.py:244
    if params.get("da") is None or params["da"].shape != da.shape:
        params["da"], params["db"] = da, db
    else:
        params["da"][...] = da
        params["db"][...] = db


class _Bound:
    """Context that yields (engine, set_id) for a trials argument.

    DeviceTrials: the resident engine, parameters pushed.  Plain list: a
    temporary engine -- upload on enter, download into the dicts on exit.
    """

    def __init__(self, trials, params, need_prior=True, pull=("mu", "v", "w", "dmu")):
        self.trials, self.params, self.need_prior, self.keys = trials, params, need_prior, pull
        self.temp = None

    def __enter__(self):
        tr, p = self.trials, self.params
        if isinstance(tr, DeviceTrials):
            return tr.engine, tr.set_id
        tr = list(tr)
        eng = Engine.for_params(p)
        self.temp = eng
        try:
            _push_params(eng, p)
            eng.upload(0, tr)
            if self.need_prior:
                chol = p.get("cholesky")  # may be a _LazyPrior: an empty-looking dict that answers __contains__
                chol = {} if chol is None else chol
                for T in sorted({t["y"].shape[0] for t in tr}):
                    if T not in chol:
                        raise KeyError("params['cholesky'] has no factor for length %d "
                                       "(call make_cholesky first)" % T)
                    eng.set_prior(T, chol[T])
        except Exception:
            eng.close()
            raise
        self.view = DeviceTrials(tr, eng, 0)
        return eng, 0

    def __exit__(self, et, ev, tb):
        if self.temp is not None:
            try:
                if et is None and self.keys:
                    self.view.pull(self.keys)
            finally:
                self.temp.close()
        return False


def make_cholesky(trials, params, config=None):
    """gp.make_cholesky (vlgp/gp.py:150-162) with math.ichol_gauss on the GPU.

    ``config["ichol"] == "host"`` selects the host NumPy factorisation instead
    (bit-identical pivots to the reference for bit-identical omega; see
    DESIGN.md, "pivot chaos")."""
    from . import gp as _gp

    if isinstance(trials, DeviceTrials):
        # the unit lengths of a resident set are fixed at upload: the engine holds the offsets
        # (cached per upload: np.unique over the offsets of 4000 segments is ~35 us between the H-step's last round and
        # the prior kernel, every EM iteration)
        entry = trials.engine.sets[trials.set_id]
        cached = getattr(trials, "_length_cache", None)
        if cached is None or cached[0] is not entry:
            cached = (entry, sorted({int(t) for t in np.unique(np.diff(np.asarray(entry[2])))}))
            trials._length_cache = cached
        lengths = cached[1]
    else:
        lengths = sorted({int(tr["y"].shape[0]) for tr in trials})
    mode = (config or {}).get("ichol", "device")
    if mode == "host":
        chol = {T: np.stack([_gp.ichol_gauss_host(T, params["omega"][l], params["rank"]) * params["sigma"][l]
                             for l in range(params["zdim"])]) for T in lengths}
        params["cholesky"] = chol
        if isinstance(trials, DeviceTrials):
            trials.engine.clear_prior()
            for T, G in chol.items():
                trials.engine.set_prior(T, G)
        return
    if isinstance(trials, DeviceTrials):
        trials.engine.build_prior(lengths, params["omega"], params["sigma"])
        params["cholesky"] = _LazyPrior(trials.engine, lengths)
        return
    with Engine.for_params(params) as eng:
        eng.build_prior(lengths, params["omega"], params["sigma"])
        params["cholesky"] = {T: eng.get_prior(T) for T in lengths}


class _LazyPrior(dict):
    """params["cholesky"] while the factors live on the device: downloads G on
    first access of a length (keeps the EM loop free of PCIe traffic)."""

    def __init__(self, engine, lengths):
        super().__init__()
        self._engine, self._lengths = engine, set(int(t) for t in lengths)

    def __missing__(self, T):
        if int(T) not in self._lengths:
            raise KeyError(T)
        G = self._engine.get_prior(int(T))
        self[int(T)] = G
        return G

    def __contains__(self, T):
        return int(T) in self._lengths

    def get(self, T, default=None):  # (dict.get bypasses __missing__)
        return self[T] if T in self else default

    def materialize(self):
        return {T: np.array(self[T]) for T in sorted(self._lengths)}

    def __reduce__(self):  # a result file must load without vlgp_amd (util.save pickles the dict): a plain dict
        return (dict, (self.materialize(),))


class _InitialPrior(dict):
    """params["initial"]["cholesky"] of a fit without a window (vlgp/api.py:60 deep-copies the full-length factors of
    the INITIAL omega, sigma): the device's copies are overwritten by the first H-step and downloading every
    full-length factor up front costs PCIe time nobody may want, so a length is factored on first access -- on the
    host, in math.ichol_gauss's own operation order (gp.ichol_gauss_host), from the initial hyperparameters kept here."""

    def __init__(self, lengths, omega, sigma, rank):
        super().__init__()
        self._lengths = sorted(int(t) for t in lengths)
        self._omega, self._sigma, self._rank = np.array(omega, dtype=float), np.array(sigma, dtype=float), int(rank)

    def __missing__(self, T):
        from . import gp as _gp

        if int(T) not in self._lengths:
            raise KeyError(T)
        G = np.stack([_gp.ichol_gauss_host(int(T), self._omega[l], self._rank) * self._sigma[l]
                      for l in range(len(self._omega))])
        self[int(T)] = G
        return G

    def __contains__(self, T):
        return int(T) in self._lengths

    def __iter__(self):
        return iter(self._lengths)

    def __len__(self):
        return len(self._lengths)

    def keys(self):
        return list(self._lengths)

    def items(self):
        return [(T, self[T]) for T in self._lengths]

    def values(self):
        return [self[T] for T in self._lengths]

    def get(self, T, default=None):  # (dict.get bypasses __missing__)
        return self[T] if T in self else default

    def __deepcopy__(self, memo):
        return _InitialPrior(self._lengths, self._omega, self._sigma, self._rank)

    def __reduce__(self):  # pickled (util.save) as the plain {T: ndarray} dict the reference's load expects
        return (dict, (dict(self.items()),))


def update_w(trials, params, config=None):
    """core.update_w (vlgp/core.py:419-442)."""
    for tr in trials:  # the reference creates missing w/v (core.py:433-434)
        if not isinstance(trials, DeviceTrials):
            tr.setdefault("w", np.zeros_like(tr["mu"]))
            tr.setdefault("v", np.zeros_like(tr["mu"]))
    with _Bound(trials, params, need_prior=False, pull=("w",)) as (eng, sid):
        eng.update_w(sid)
        TRACE["update_w"] = eng.last_estep_path


def update_v(trials, params, config):
    """core.update_v (vlgp/core.py:445-471)."""
    if config["method"] != "VB":
        return
    with _Bound(trials, params, pull=("v",)) as (eng, sid):
        bad = eng.update_v(sid, True, count=not isinstance(trials, DeviceTrials))
        TRACE["update_v"] = eng.last_estep_path
        if bad:
            logger.error("Singular I + G'WG in %d unit-latent pairs", bad)


def estep(trials, params, config):
    """core.estep (vlgp/core.py:123-126): config["Eniter"] inner iterations per unit."""
    if config["Eniter"] < 1:
        return
    with _Bound(trials, params) as (eng, sid):
        bad = eng.estep(sid, config["Eniter"], config["dmu_bound"], config["method"] == "VB",
                        count=not isinstance(trials, DeviceTrials))
        TRACE["estep"] = eng.last_estep_path
        if bad:
            logger.error("%d posterior updates hit a singular system and were zeroed", bad)


def mstep(trials, params, config):
    """core.mstep (vlgp/core.py:129-249)."""
    if config["Mniter"] < 1:
        return
    if params.get("da") is None:
        params["da"] = np.zeros_like(params["a"])
        params["db"] = np.zeros_like(params["b"])
    with _Bound(trials, params, need_prior=False, pull=()) as (eng, sid):
        bad = eng.mstep(sid, config["Mniter"], config["use_hessian"], config["eps"],
                        config["learning_rate"], config["da_bound"], config["db_bound"],
                        count=not isinstance(trials, DeviceTrials))
        if bad:
            logger.error("%d Newton systems were singular (gradient step taken)", bad)
        _pull_params(eng, params)


def hstep(trials, params, config):
    """core.hstep (vlgp/core.py:252-257)."""
    if not config["Hstep"]:
        return
    from . import gp as _gp

    _gp.optimize(trials, params, config)


def infer(trials, params, config, echo=None):
    """core.infer (vlgp/core.py:260-266): E-step with Eniter := max_iter."""
    keep = config["Eniter"]
    config["Eniter"] = config["max_iter"]
    t0 = time.perf_counter()
    try:
        estep(trials, params, config)
        if isinstance(trials, DeviceTrials):
            trials.engine.synchronize()
    finally:
        config["Eniter"] = keep
    if echo:
        echo("{:.2f}s".format(time.perf_counter() - t0))


def constrain_loading(trials, params, config):
    """core.constrain_loading (vlgp/core.py:392-416)."""
    kind = config["constrain_loading"]
    if not kind or kind == "none":
        return
    a = params["a"]
    L = a.shape[0]
    if kind == "svd":
        _, _, vt = np.linalg.svd(a, full_matrices=False)
        mat = a @ vt.T
        params["a"] = vt
    else:
        if kind == "fro":
            s = np.full(L, np.linalg.norm(a, ord="fro") + config["eps"])
        else:
            s = np.linalg.norm(a, ord=kind, axis=1) + config["eps"]
        params["a"] /= s[:, None]
        mat = np.diag(s)
    if isinstance(trials, DeviceTrials):
        if kind == "svd" and getattr(trials, "parent_set", None) is not None and not trials.detached:
            # the reference REBINDS every segment's mu here (core.py:407-408): from now on the segments no longer
            # write through to their trials, whose mu stays what it is at this moment (fit's final inference
            # starts from it).  Keep that copy; FitSession.finish puts it back after the merge.
            trials.engine.stash_mu(trials.parent_set)
            trials.detached = True
            if trials.unit_of is not None:  # overlapping segments stop sharing their mu rows (v stays shared)
                trials.engine.unshare_mu(trials.set_id)
        trials.engine.apply_latent_map(trials.set_id, mat)
        trials.engine.set_loading(params["a"])  # b and noise are untouched by this constraint
    else:
        for tr in trials:
            tr["mu"] = tr["mu"] @ mat if kind == "svd" else _imul_cols(tr["mu"], np.diag(mat))


def _imul_cols(mu, s):
    mu *= s
    return mu


def constrain_latent(trials, params, config):
    """core.constrain_latent (vlgp/core.py:366-389); off by default."""
    kind = config["constrain_latent"]
    if not kind or kind == "none":
        return
    L = params["zdim"]
    if isinstance(trials, DeviceTrials):
        s1, s2, cnt = trials.engine.latent_moments(trials.set_id)
        mean = s1 / cnt
        std = np.sqrt(np.maximum(s2 / cnt - mean ** 2, 0.0))
    else:
        mu = np.concatenate([tr["mu"] for tr in trials], axis=0)
        mean, std = mu.mean(axis=0), mu.std(axis=0)
    shift = np.zeros(L)
    scale = np.ones(L)
    if kind in ("location", "both"):
        shift = mean
        params["b"][0, :] += mean @ params["a"]
    if kind in ("scale", "both"):
        scale = 1.0 / std
        params["a"] *= std[:, None]
    if isinstance(trials, DeviceTrials):
        if trials.unit_of is not None and kind == "both":
            # overlapping segments: the reference shifts every segment, THEN scales every segment (core.py:377-388); a
            # shared row sees each pass twice, so the two passes cannot be folded into one affine map
            trials.engine.apply_latent_map(trials.set_id, np.eye(L), shift)
            trials.engine.apply_latent_map(trials.set_id, np.diag(scale))
        else:
            trials.engine.apply_latent_map(trials.set_id, np.diag(scale), shift)
        _push_params(trials.engine, params)
    else:
        for tr in trials:
            tr["mu"] -= shift
            tr["mu"] *= scale


def new_runtime():
    return {"it": 0, "e_elapsed": [], "m_elapsed": [], "h_elapsed": [], "em_elapsed": []}


def _elbo_totals(eng, sid, vb):
    """[elbo, ell, kl] of this rank's units of set ``sid`` (evaluation.elbo_from_terms; NaN elbo / kl under MAP)."""
    from .evaluation import elbo_from_terms

    sums, terms, bad, _ = eng.elbo(sid, vb)
    out = elbo_from_terms(sums, terms, eng.unit_ranks(sid), vb=vb, n_failed=bad)
    return np.array([out["elbo"], out["ell"], float(np.sum(out["kl"]))])


def em_iteration(trials, params, config, runtime, echo=None, track_elbo=False):
    """One pass of the body of core.vem (vlgp/core.py:298-357): E, M, H, timers,
    callbacks, convergence test.  Returns True when the stopping rule fires.

    ``track_elbo``: after the E-step -- the posterior fresh, the parameters and the prior those the E-step used -- the
    variational lower bound of the unit set is appended to ``runtime["elbo"]`` (its expected log-likelihood and KL
    totals to ``runtime["elbo_ell"]``, ``runtime["elbo_kl"]``), summed over the ranks.  The units are the segments of
    the cut, and segments of one trial may overlap: the trace is the objective of the SEGMENT SET, not of the trials.
    The M-step is then enqueued after the E-step instead of under it (it would change a, b under the evaluation);
    the iteration computes the same bits either way."""
    eng, sid = trials.engine, trials.set_id
    tol = config["tol"]
    runtime["it"] += 1
    # pre-iteration norm of mu (core.py:300-305): the value the previous iteration's closing norms call returned,
    # when nothing has touched the set since (one kernel + one device -> host copy less per iteration)
    cached = getattr(trials, "_norm_cache", None)
    if cached is not None and cached[0] == (eng.state_epoch, sid):
        norm_mu = cached[1]
    else:
        norm_mu, _ = eng.norms(sid)
    trials._norm_cache = None
    norm_a = np.linalg.norm(params["a"])
    norm_b = np.linalg.norm(params["b"])

    t0 = time.perf_counter()
    constrain_loading(trials, params, config)
    estep(trials, params, config)
    # M and H are independent given the posterior (M: a, b from mu, v; H: omega from
    # mu, w): the M-step is enqueued on the engine's second stream and runs under the
    # H-step's host-driven rounds.  m_elapsed is the M-step's device time, h_elapsed
    # the wall time of the H-step, em_elapsed the wall time of the whole iteration.
    m_ms = 0.0
    m_async = config["Mniter"] >= 1
    latent_constraint = bool(config["constrain_latent"]) and config["constrain_latent"] != "none"

    def begin_m():
        if params.get("da") is None:
            params["da"] = np.zeros_like(params["a"])
            params["db"] = np.zeros_like(params["b"])
        eng.mstep_begin(sid, config["Mniter"], config["use_hessian"], config["eps"], config["learning_rate"],
                        config["da_bound"], config["db_bound"])

    # the M-step lane waits for the E-step on the device (an event): its ~50 launches are enqueued (one graph launch,
    # ~80 us of host time) while the E-step still runs, unless constrain_latent has to touch mu, a, b in between
    early_m = m_async and not latent_constraint and not track_elbo
    if early_m:
        begin_m()
    m_first = m_async and ((eng.world > 1 and not eng.host_exchange) or bool(os.environ.get("VLGP_M_SEQUENTIAL")))

    # mu, dmu and w are final once the E-step (and constrain_latent) are done -- the M-step writes a, b; the H-step omega:
    # the sums of the stopping rule (core.py:350-354) and the H-step's moments of mu / copy of w are queued behind the
    # E-step while it still runs: nothing the host has to do between the E-step's end and the first round
    prepare = bool(config["Hstep"]) and bool(config.get("window")) and not m_first

    def after_estep():
        eng.norms_begin(sid)
        if prepare:
            eng.hstep_prepare(sid, config["window"])

    if not latent_constraint:
        after_estep()
    eng.estep_wait()   # the E-step alone: neither the M-step lane nor what is queued behind it
    t1 = time.perf_counter()
    elbo_now = _elbo_totals(eng, sid, config["method"] == "VB") if track_elbo else None
    constrain_latent(trials, params, config)
    if latent_constraint:
        after_estep()
    norms_epoch = eng.state_epoch
    if m_async and not early_m:
        begin_m()

    def finish_m():
        bad, ms = eng.mstep_end()
        if bad:
            logger.error("%d Newton systems were singular (gradient step taken)", bad)
        _pull_params(eng, params)
        return ms

    # With several ranks the M-step lane issues RCCL all-reduces on its own communicator.  That is safe
    # under the H-step only when the H-step issues none itself, i.e. when its round sums are exchanged on
    # the host (Engine.host_exchange); otherwise two communicators would be in flight with no common
    # order across ranks, and the M-step is finished first.
    if m_first:
        m_ms = finish_m()
        m_async = False
    t2 = time.perf_counter()
    hstep(trials, params, config)  # every objective round ends with a device -> host copy: no extra sync
    t3 = time.perf_counter()
    if m_async:
        m_ms = finish_m()
    t4 = time.perf_counter()

    runtime["e_elapsed"].append(t1 - t0)
    runtime["m_elapsed"].append(m_ms * 1e-3)
    runtime["h_elapsed"].append(t3 - t2)
    runtime["em_elapsed"].append(t4 - t0)
    config["runtime"] = runtime
    if echo:
        echo("Iteration {:4d}, E-step {:.2f}s, M-step {:.2f}s".format(
            runtime["it"], runtime["e_elapsed"][-1], runtime["m_elapsed"][-1]))

    norm_mu_now, norm_dmu = eng.norms_end()
    if track_elbo:
        if eng.world > 1:  # (here, with no lane in flight: every rank reports the sum over the ranks)
            eng.allreduce_host(elbo_now)
        for key, val in zip(("elbo", "elbo_ell", "elbo_kl"), elbo_now):
            runtime.setdefault(key, []).append(float(val))
    if config["callbacks"]:
        trials.pull()
        for cb in config["callbacks"]:
            try:
                cb(trials, params, config)
            except RuntimeError:
                logger.error("Callback {} failed".format(cb))
        if eng.state_epoch != norms_epoch:  # a callback changed the units: the reference takes the norms after it
            norm_mu_now, norm_dmu = eng.norms(sid)
    trials._norm_cache = ((eng.state_epoch, sid), norm_mu_now)
    converged = (norm_dmu < tol * norm_mu
                 and np.linalg.norm(params["da"]) < tol * norm_a
                 and np.linalg.norm(params["db"]) < tol * norm_b)
    return bool(converged and runtime["it"] >= config["min_iter"])


def vem(trials, params, config, echo=None):
    """core.vem (vlgp/core.py:269-359): the EM loop, timers and stopping rule.

    Timers are wall-clock around device-synchronised phases, so
    ``config["runtime"]`` means what it means in the reference.
    """
    if not isinstance(trials, DeviceTrials):
        raise TypeError("vem runs on DeviceTrials (use vlgp_amd.fit, or Engine + DeviceTrials)")
    runtime = new_runtime()
    _push_params(trials.engine, params)
    for _ in range(config["max_iter"]):
        if em_iteration(trials, params, config, runtime, echo):
            break
