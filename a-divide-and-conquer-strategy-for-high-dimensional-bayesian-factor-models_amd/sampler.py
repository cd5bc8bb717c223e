"""Handle wrapper around the C ABI: the hot loop of divideconquer.m (dc:90-197).

Arrays cross the boundary in the reference's MATLAB shapes and column-major
order (``Lambda`` P x K x g_local, ``Yd`` n x P x g_local, ``delta`` K x 1 x g,
...), exactly as a MEX gateway would pass them.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _abi

STATE_FIELDS = ("Lambda", "ps", "omega", "psi", "Plam", "X", "Z", "eta", "delta", "tauh")


@dataclass(frozen=True)
class Hyper:
    """dc:62-65 (hard-coded in the reference)."""
    as_: float = 1.0
    bs: float = 0.3
    df: float = 3.0
    ad1: float = 2.0
    bd1: float = 1.0
    ad2: float = 2.0
    bd2: float = 1.0


def _f64F(a) -> np.ndarray:
    return np.asfortranarray(np.asarray(a, dtype=np.float64))


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Sampler:
    """One rank's handle: shards [rank*g_local, (rank+1)*g_local) of a chain."""

    def __init__(self, n, P, g, K, rho, burnin, mcmc, thin, *, hyper: Hyper = Hyper(), seed=0,
                 nranks=1, rank=0, device=0, inject_draws=False, asm_batch=0, flags=0, sigma_m2=False,
                 precision_mean=False, partial_corr=False, corr=False, regression=False):
        self.lib = _abi.load_library()
        cfg = _abi.DcfmConfig()
        cfg.n, cfg.P, cfg.g, cfg.K = int(n), int(P), int(g), int(K)
        cfg.rho = float(rho)
        cfg.burnin, cfg.mcmc, cfg.thin = int(burnin), int(mcmc), int(thin)
        cfg.as_, cfg.bs, cfg.df = hyper.as_, hyper.bs, hyper.df
        cfg.ad1, cfg.bd1, cfg.ad2, cfg.bd2 = hyper.ad1, hyper.bd1, hyper.ad2, hyper.bd2
        cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        cfg.nranks, cfg.rank, cfg.device = int(nranks), int(rank), int(device)
        cfg.flags = ((_abi.DCFM_FLAG_INJECT_DRAWS if inject_draws else 0) |
                     (_abi.DCFM_FLAG_SIGMA_M2 if sigma_m2 else 0) |
                     (_abi.DCFM_FLAG_PRECISION_MEAN if precision_mean else 0) |
                     (_abi.DCFM_FLAG_PARTIAL_CORR if partial_corr else 0) |
                     (_abi.DCFM_FLAG_CORR if corr else 0) |
                     (_abi.DCFM_FLAG_REGRESSION if regression else 0) | int(flags))
        cfg.asm_batch = int(asm_batch)
        self.cfg = cfg
        h = C.c_void_p()
        rc = self.lib.dcfm_create(C.byref(cfg), C.byref(h))
        _abi.check(self.lib, None, rc)
        self.h = h
        self.n, self.P, self.g, self.K = cfg.n, cfg.P, cfg.g, cfg.K
        self.nranks, self.rank = cfg.nranks, cfg.rank
        self.g_local = self.g // self.nranks
        self.shard0 = self.rank * self.g_local

    # -- lifecycle -------------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.dcfm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        _abi.check(self.lib, self.h, rc)

    # -- multi-rank -------------------------------------------------------------
    @staticmethod
    def unique_id() -> bytes:
        lib = _abi.load_library()
        buf = (C.c_uint8 * 128)()
        _abi.check(lib, None, lib.dcfm_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, uid: bytes):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._check(self.lib.dcfm_comm_init(self.h, buf))

    # -- inputs ----------------------------------------------------------------
    @staticmethod
    def comm_loopback(samplers):
        """In-process loopback communicator over ``samplers`` (ranks 0..n-1 of one chain
        on one device): each sampler must then be driven from its own thread."""
        n = len(samplers)
        arr = (C.c_void_p * n)(*[s_.h.value for s_ in samplers])
        lib = samplers[0].lib
        _abi.check(lib, None, lib.dcfm_comm_init_loopback(arr, n))

    def set_data(self, Yd_local):
        Y = _f64F(Yd_local)
        if Y.shape != (self.n, self.P, self.g_local):
            raise ValueError(f"Yd_local must be n x P x g_local = {(self.n, self.P, self.g_local)}, got {Y.shape}")
        self._miss_mask = None                                       # the mask of set_missing goes with the data
        self._check(self.lib.dcfm_set_data(self.h, _ptr(Y)))

    def set_data_raw(self, Y, cols):
        """On-device ingest (dc:48-59, dcfm_set_data_raw): Y is the raw n x p_in data,
        ``cols`` the 0-based input column of every (local shard, position) pair, length
        P * g_local (``shard_columns``).  Returns (sd, kernel_ms): the P x g_local sample
        standard deviations and the standardise kernel's device time."""
        Y = _f64F(Y)
        if Y.ndim != 2 or Y.shape[0] != self.n:
            raise ValueError(f"Y must be n x p_in with n = {self.n}, got {Y.shape}")
        c = np.ascontiguousarray(np.asarray(cols, dtype=np.int64).reshape(-1))
        if c.size != self.P * self.g_local:
            raise ValueError(f"cols must hold P * g_local = {self.P * self.g_local} indices, got {c.size}")
        sd = np.zeros((self.P, self.g_local), dtype=np.float64, order="F")
        ms = C.c_double(0.0)
        self._miss_mask = None
        self._check(self.lib.dcfm_set_data_raw(self.h, _ptr(Y), Y.shape[1],
                                               c.ctypes.data_as(C.POINTER(C.c_int64)), _ptr(sd), C.byref(ms)))
        return sd, ms.value

    def get_data(self) -> np.ndarray:
        """Yd as the sweep holds it (n x P x g_local)."""
        out = np.zeros((self.n, self.P, self.g_local), dtype=np.float64, order="F")
        self._check(self.lib.dcfm_get_data(self.h, _ptr(out)))
        return out

    def _shapes(self):
        n, P, K, gl, g = self.n, self.P, self.K, self.g_local, self.g
        return {"Lambda": (P, K, gl), "ps": (P, 1, gl), "omega": (P, gl), "psi": (P, K, gl),
                "Plam": (P, K, gl), "X": (n, K), "Z": (n, K, gl), "eta": (n, K, gl),
                "delta": (K, 1, g), "tauh": (K, 1, g)}

    def set_state(self, state: dict):
        """state: MATLAB-shaped arrays; local shards for per-shard fields, all g for delta/tauh."""
        shapes = self._shapes()
        keep = []
        view = _abi.DcfmStateView()
        for f in STATE_FIELDS:
            if f == "eta":
                continue
            a = _f64F(state[f])
            if a.size != int(np.prod(shapes[f])):
                raise ValueError(f"{f}: expected shape {shapes[f]}, got {a.shape}")
            keep.append(a)
            setattr(view, f, _ptr(a))
        self._check(self.lib.dcfm_set_state(self.h, C.byref(view)))

    def init_state(self):
        """dc:68-87 on the device from the Philox stream (dcfm_init_state), instead of set_state."""
        self._check(self.lib.dcfm_init_state(self.h))

    def set_draws(self, draws: dict, first_iter: int, n_iter: int):
        """draws: full-g arrays NZ (K,n,g,T), NX (K,n,T), NL (K,P,g,T), Gpsi (P,K,g,T),
        Gdelta (K,g,T), Gps (P,g,T) — the layout of oracle.IterDraws.stacked()."""
        view = _abi.DcfmDrawsView()
        keep = []
        for f in ("NZ", "NX", "NL", "Gpsi", "Gdelta", "Gps"):
            a = _f64F(draws[f])
            keep.append(a)
            setattr(view, f, _ptr(a))
        self._check(self.lib.dcfm_set_draws(self.h, C.byref(view), int(first_iter), int(n_iter)))

    # -- hot loop ----------------------------------------------------------------
    def run(self, first_iter: int, n_iter: int):
        self._check(self.lib.dcfm_run(self.h, int(first_iter), int(n_iter)))

    def synchronize(self):
        self._check(self.lib.dcfm_synchronize(self.h))

    # -- outputs -------------------------------------------------------------------
    def get_state(self, fields=STATE_FIELDS, raw=False) -> dict:
        """The state in MATLAB shapes.  ``raw``: skip the non-finite check (dcfm_get_state_raw), to
        read the state after a run that ended in DCFM_ERR_NUMERIC."""
        shapes = self._shapes()
        out = {f: np.zeros(shapes[f], dtype=np.float64, order="F") for f in fields}
        view = _abi.DcfmStateView()
        for f, a in out.items():
            setattr(view, f, _ptr(a))
        fn = self.lib.dcfm_get_state_raw if raw else self.lib.dcfm_get_state
        self._check(fn(self.h, C.byref(view)))
        return out

    def get_sigma(self):
        """Sigmaout (p x p, Fortran order).  Collective when nranks > 1: every rank calls it,
        rank 0 receives the matrix and the other ranks get None (Sigmaout is block-sharded
        over the ranks, dcfm_sigma_block; each element moves once, owner -> rank 0)."""
        p = self.P * self.g
        if self.rank != 0:
            self._check(self.lib.dcfm_get_sigma(self.h, None))
            return None
        S = np.zeros((p, p), dtype=np.float64, order="F")
        self._check(self.lib.dcfm_get_sigma(self.h, _ptr(S)))
        return S

    def get_sigma_cols(self, col0: int, ncols: int):
        """Sigmaout(:, col0 : col0+ncols) as a p x ncols Fortran array (collective if nranks > 1;
        rank 0 receives it, other ranks get None)."""
        p = self.P * self.g
        if self.rank != 0:
            self._check(self.lib.dcfm_get_sigma_cols(self.h, int(col0), int(ncols), None))
            return None
        S = np.zeros((p, int(ncols)), dtype=np.float64, order="F")
        self._check(self.lib.dcfm_get_sigma_cols(self.h, int(col0), int(ncols), _ptr(S)))
        return S

    @staticmethod
    def _moment(which) -> int:
        if isinstance(which, str):
            if which not in _abi.SIGMA_MOMENTS:
                raise ValueError(f"which must be one of {sorted(_abi.SIGMA_MOMENTS)}, got {which!r}")
            return _abi.SIGMA_MOMENTS[which]
        return int(which)

    def get_sigma_moment(self, which):
        """A posterior moment of Sigma's entries (p x p, Fortran order): ``"mean"`` = get_sigma(),
        ``"m2"`` the element-wise second moment of the per-sample Sigma (1/effsamp scaling, as the
        mean), ``"sd"`` the posterior standard deviation over the samples saved so far (population
        form).  ``"m2"`` / ``"sd"`` need ``sigma_m2=True``.  Collective like get_sigma()."""
        w = self._moment(which)
        p = self.P * self.g
        if self.rank != 0:
            self._check(self.lib.dcfm_get_sigma_moment(self.h, w, None))
            return None
        S = np.zeros((p, p), dtype=np.float64, order="F")
        self._check(self.lib.dcfm_get_sigma_moment(self.h, w, _ptr(S)))
        return S

    def get_sigma_moment_cols(self, which, col0: int, ncols: int):
        """Columns [col0, col0+ncols) of get_sigma_moment(which), p x ncols (as get_sigma_cols)."""
        w = self._moment(which)
        p = self.P * self.g
        if self.rank != 0:
            self._check(self.lib.dcfm_get_sigma_moment_cols(self.h, w, int(col0), int(ncols), None))
            return None
        S = np.zeros((p, int(ncols)), dtype=np.float64, order="F")
        self._check(self.lib.dcfm_get_sigma_moment_cols(self.h, w, int(col0), int(ncols), _ptr(S)))
        return S

    def get_precision_mean(self):
        """The posterior mean of the precision matrix, ``(1/effsamp) sum_s inv(Sigma(s))`` over the saved
        samples (p x p, Fortran order, Sigmaout's coordinates and 1/effsamp scaling; all zeros before the
        first saved sample).  E[inv(Sigma)], not ``inv(get_sigma())``.  Needs ``precision_mean=True``.
        Symmetric bit for bit.  Collective like get_sigma(): rank 0 receives it, the others get None."""
        p = self.P * self.g
        if self.rank != 0:
            self._check(self.lib.dcfm_get_precision_mean(self.h, None))
            return None
        T = np.zeros((p, p), dtype=np.float64, order="F")
        self._check(self.lib.dcfm_get_precision_mean(self.h, _ptr(T)))
        return T

    def get_precision_mean_cols(self, col0: int, ncols: int):
        """Columns [col0, col0+ncols) of get_precision_mean(), p x ncols (as get_sigma_cols)."""
        p = self.P * self.g
        if self.rank != 0:
            self._check(self.lib.dcfm_get_precision_mean_cols(self.h, int(col0), int(ncols), None))
            return None
        T = np.zeros((p, int(ncols)), dtype=np.float64, order="F")
        self._check(self.lib.dcfm_get_precision_mean_cols(self.h, int(col0), int(ncols), _ptr(T)))
        return T

    def get_partial_corr(self, which="mean"):
        """A posterior moment of the partial correlations (p x p, Fortran order, Sigmaout's coordinates).  Per
        saved sample ``R(s)_ab = -T_ab / sqrt(T_aa T_bb)``, ``T = inv(Sigma(s))``, with a unit diagonal; ``"mean"``
        is ``(1/effsamp) sum_s R(s)`` (diagonal exactly saved/effsamp), ``"m2"`` the same sum of ``R(s)**2``,
        ``"sd"`` the posterior standard deviation over the samples saved so far (population form, 0 on the
        diagonal).  The posterior mean of the partial correlation, not the plug-in
        ``diagnostics.partial_correlations(get_precision_mean())``.  Needs ``partial_corr=True``.  Symmetric bit
        for bit.  Collective like get_sigma(): rank 0 receives it, the others get None."""
        w = self._moment(which)
        p = self.P * self.g
        if self.rank != 0:
            self._check(self.lib.dcfm_get_partial_corr(self.h, w, None))
            return None
        R = np.zeros((p, p), dtype=np.float64, order="F")
        self._check(self.lib.dcfm_get_partial_corr(self.h, w, _ptr(R)))
        return R

    def get_partial_corr_cols(self, which, col0: int, ncols: int):
        """Columns [col0, col0+ncols) of get_partial_corr(which), p x ncols (as get_sigma_cols)."""
        w = self._moment(which)
        p = self.P * self.g
        if self.rank != 0:
            self._check(self.lib.dcfm_get_partial_corr_cols(self.h, w, int(col0), int(ncols), None))
            return None
        R = np.zeros((p, int(ncols)), dtype=np.float64, order="F")
        self._check(self.lib.dcfm_get_partial_corr_cols(self.h, w, int(col0), int(ncols), _ptr(R)))
        return R

    def get_corr(self, which="mean"):
        """A posterior moment of the correlation matrix (p x p, Fortran order, Sigmaout's coordinates).  Per saved
        sample ``R(s) = Sigma(s) / sqrt(v v')``, ``v = diag(Sigma(s))``, with a unit diagonal; ``"mean"`` is
        ``(1/effsamp) sum_s R(s)`` (diagonal exactly saved/effsamp), ``"m2"`` the same sum of ``R(s)**2``, ``"sd"``
        the posterior standard deviation over the samples saved so far (population form, 0 on the diagonal).
        The posterior mean of the correlation, not the plug-in ``diagnostics.correlation(get_sigma())``.  Needs
        ``corr=True``.  Symmetric bit for bit.  Collective like get_sigma(): rank 0 receives it, the others get
        None."""
        w = self._moment(which)
        p = self.P * self.g
        if self.rank != 0:
            self._check(self.lib.dcfm_get_corr(self.h, w, None))
            return None
        R = np.zeros((p, p), dtype=np.float64, order="F")
        self._check(self.lib.dcfm_get_corr(self.h, w, _ptr(R)))
        return R

    def get_corr_cols(self, which, col0: int, ncols: int):
        """Columns [col0, col0+ncols) of get_corr(which), p x ncols (as get_sigma_cols)."""
        w = self._moment(which)
        p = self.P * self.g
        if self.rank != 0:
            self._check(self.lib.dcfm_get_corr_cols(self.h, w, int(col0), int(ncols), None))
            return None
        R = np.zeros((p, int(ncols)), dtype=np.float64, order="F")
        self._check(self.lib.dcfm_get_corr_cols(self.h, w, int(col0), int(ncols), _ptr(R)))
        return R

    def get_communality(self, which="mean"):
        """A posterior moment of the communalities ``h_a(s) = |Lambda_a(s)|^2 / (|Lambda_a(s)|^2 + omega_a(s))``,
        the share of each variable's variance that the factors explain (p entries, Sigmaout's coordinates):
        ``"mean"`` ``(1/effsamp) sum_s h(s)``, ``"m2"`` the same sum of ``h(s)**2``, ``"sd"`` the posterior
        standard deviation over the samples saved so far (population form).  Needs ``corr=True``.  Not
        collective: every rank holds all p entries."""
        w = self._moment(which)
        hv = np.zeros(self.P * self.g, dtype=np.float64)
        self._check(self.lib.dcfm_get_communality(self.h, w, _ptr(hv)))
        return hv

    def sigma_block(self) -> dict:
        """This rank's block of Sigmaout: rows [row0, row1) of the lower triangle and its bytes
        (the mean, plus the second moment with ``sigma_m2``, the precision mean with ``precision_mean``, the
        two moments of the partial correlations with ``partial_corr`` and those of the correlations with
        ``corr``)."""
        out = (C.c_int64 * 3)()
        self._check(self.lib.dcfm_sigma_block(self.h, out))
        return {"row0": int(out[0]), "row1": int(out[1]), "bytes": int(out[2])}

    def sigma_error(self, U, s, iters: int = 60, seed: int = 1) -> dict:
        """Frobenius / operator-norm error of Sigmaout against U U' + diag(s), on the device
        (dcfm_sigma_error).  U: p x r truth factors in output coordinates, s: p."""
        p = self.P * self.g
        U = _f64F(np.asarray(U, dtype=np.float64).reshape(p, -1))
        s = _f64F(np.asarray(s, dtype=np.float64).reshape(p))
        out = np.zeros(3)
        self._check(self.lib.dcfm_sigma_error(self.h, _ptr(U), U.shape[1], _ptr(s), int(iters),
                                              int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(out)))
        fro, tru, op = (float(x) for x in out)
        return {"fro": fro, "op": op, "fro_rel": fro / tru if tru > 0 else float("nan"), "truth_fro": tru}

    def sigma_apply(self, V, return_ms=False):
        """Sigmaout @ V on the device (dcfm_sigma_apply): V is (p,) or (p, nv) in Sigmaout's permuted,
        standardised coordinates, the result has V's shape and equals ``get_sigma() @ V`` without the
        matrix leaving HBM.  Any nv; the kernel serves 32 columns per pass.  Collective when
        nranks > 1: every rank calls it with the same V and receives the full product.
        ``return_ms``: also the kernels' accumulated device time in milliseconds."""
        p = self.P * self.g
        V = np.asarray(V, dtype=np.float64)
        if V.ndim not in (1, 2) or V.shape[0] != p:
            raise ValueError(f"V must be (p,) or (p, nv) with p = {p}, got {V.shape}")
        V2 = _f64F(V.reshape(p, -1))
        out = np.zeros(V2.shape, dtype=np.float64, order="F")
        ms = C.c_double(0.0)
        self._check(self.lib.dcfm_sigma_apply(self.h, _ptr(V2), V2.shape[1], _ptr(out),
                                              C.byref(ms) if return_ms else None))
        out = out.reshape(V.shape, order="F")
        return (out, ms.value) if return_ms else out

    def sigma_eigs(self, r, tol=1e-10, max_passes=None, seed=1, vectors=True) -> dict:
        """The r largest eigenpairs of Sigmaout (1 <= r <= min(32, p)) by a block Krylov iteration on
        sigma_apply (dcfm_sigma_eigs); Sigmaout stays in HBM.  Returns ``values`` (r, descending),
        ``vectors`` (p x r, orthonormal columns, the entry of largest magnitude of each positive; None
        with ``vectors=False``), ``resid`` (||Sigma v_i - lambda_i v_i||_2 from a real pass on the
        returned vectors), ``passes`` (block applies of the iteration) and ``converged`` = all resid
        <= tol * values[0].  Reaching ``max_passes`` (default ceil(p / b) + 1 with b = min(32, p),
        enough for the basis to span everything) unconverged is not an error: read ``resid``.
        Collective when nranks > 1; every rank returns the same bits."""
        p = self.P * self.g
        r = int(r)
        b = min(32, p)
        if max_passes is None:
            max_passes = -(-p // b) + 1
        vals = np.zeros(max(r, 1))
        res = np.zeros(max(r, 1))
        vec = np.zeros((p, max(r, 1)), dtype=np.float64, order="F") if vectors else None
        npass = C.c_int32(0)
        self._check(self.lib.dcfm_sigma_eigs(self.h, r, float(tol), int(max_passes), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                             _ptr(vals), _ptr(vec) if vectors else None, _ptr(res), C.byref(npass)))
        return {"values": vals, "vectors": vec, "resid": res, "passes": int(npass.value),
                "converged": bool(np.all(res <= float(tol) * vals[0]))}

    def sigma_solve(self, B, tol=1e-10, max_iter=None, return_info=False):
        """Sigmaout^{-1} B on the device (dcfm_sigma_solve): B is (p,) or (p, nv) in Sigmaout's permuted,
        standardised coordinates and X has B's shape, ``get_sigma() @ X = B`` without the matrix leaving
        HBM.  Conjugate gradients, every column on its own (alpha, beta and stop test per column), 32
        columns per pass and the whole iteration on the device.  A column stops when its recurrence
        residual is <= tol * ||B_c||, or after ``max_iter`` steps (default min(2 p, 1000)); reaching
        ``max_iter`` is not an error: read ``relres``.  Collective when nranks > 1: every rank calls it
        with the same B and receives the same X.
        ``return_info``: also a dict with ``relres`` (||B_c - Sigma X_c|| / ||B_c|| from a real pass on
        the returned X; 0 for a zero column), ``iters`` (CG steps of each column), ``quad`` (B_c' X_c,
        the quadratic form b' Sigma^{-1} b), ``converged`` (``iters < max_iter``: the column was stopped
        by its own test, or by the zero-denominator guard, before the cap -- a column that met the test
        on the very last allowed step counts as not converged; ``relres`` is the measure) and ``ms``
        (the kernels' accumulated device time).  The per-column entries have shape (nv,), or are
        scalars for a (p,) B."""
        p = self.P * self.g
        B = np.asarray(B, dtype=np.float64)
        if B.ndim not in (1, 2) or B.shape[0] != p:
            raise ValueError(f"B must be (p,) or (p, nv) with p = {p}, got {B.shape}")
        B2 = _f64F(B.reshape(p, -1))
        nv = B2.shape[1]
        if max_iter is None:
            max_iter = min(2 * p, 1000)
        X = np.zeros(B2.shape, dtype=np.float64, order="F")
        relres, quad = np.zeros(max(nv, 1)), np.zeros(max(nv, 1))
        iters = np.zeros(max(nv, 1), dtype=np.int32)
        ms = C.c_double(0.0)
        self._check(self.lib.dcfm_sigma_solve(self.h, _ptr(B2), nv, float(tol), int(max_iter), _ptr(X), _ptr(relres),
                                              iters.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(quad),
                                              C.byref(ms) if return_info else None))
        X = X.reshape(B.shape, order="F")
        if not return_info:
            return X
        info = {"relres": relres, "iters": iters.astype(np.int64), "quad": quad, "converged": iters < int(max_iter)}
        if B.ndim == 1:
            info = {k: v[0].item() for k, v in info.items()}
        info["ms"] = ms.value
        return X, info

    def saved_samples(self) -> int:
        return int(self.lib.dcfm_saved_samples(self.h))

    # -- chain trace (diagnostics across chains) -----------------------------------
    TRACE_FIELDS = ("lambda_fro2", "tr_omega", "sum_log_ps", "sum_log_tau")

    def set_trace(self, capacity: int):
        """Record one row of TRACE_FIELDS per iteration of later runs (0 = off)."""
        self._check(self.lib.dcfm_set_trace(self.h, int(capacity)))
        self._trace_cap = int(capacity)

    def get_trace(self) -> np.ndarray:
        """(iterations recorded) x 4 array of this rank's local-shard sums."""
        cnt = C.c_int64(0)
        cap = getattr(self, "_trace_cap", 0)
        out = np.zeros((max(cap, 1), 4), dtype=np.float64)
        self._check(self.lib.dcfm_get_trace(self.h, _ptr(out), C.byref(cnt)))
        return out[:cnt.value].copy()

    # -- per-sample probe draws ------------------------------------------------------
    def set_probes(self, V, capacity=None):
        """Record ``V' Sigma(s) V`` for every saved sample s of later runs (dcfm_set_probes): V is
        (p,) or (p, nv), 1 <= nv <= 32, in Sigmaout's permuted, standardised coordinates (every rank
        passes the same V).  Up to ``capacity`` draws are held (default ``mcmc // thin``); later saved
        samples are not recorded.  Calling it again replaces V and resets the count; ``set_probes(None)``
        turns the recording off and frees its buffers."""
        if V is None:
            self._check(self.lib.dcfm_set_probes(self.h, None, 0, 0))
            self._probe_nv = self._probe_cap = 0
            return
        p = self.P * self.g
        V = np.asarray(V, dtype=np.float64)
        if V.ndim not in (1, 2) or V.shape[0] != p:
            raise ValueError(f"V must be (p,) or (p, nv) with p = {p}, got {V.shape}")
        V2 = _f64F(V.reshape(p, -1))
        if capacity is None:
            capacity = int(self.cfg.mcmc) // int(self.cfg.thin)
        self._check(self.lib.dcfm_set_probes(self.h, _ptr(V2), V2.shape[1], int(capacity)))
        self._probe_nv = V2.shape[1] if int(capacity) > 0 else 0
        self._probe_cap = int(capacity)

    def probe_draws(self) -> np.ndarray:
        """The recorded draws, shape (S, nv, nv): ``draws[s] = V' Sigma(s) V`` in saved-sample order, the
        per-sample matrix without effsamp scaling (``draws.sum(0) / effsamp = V' Sigmaout V``), every
        slice symmetric bit for bit.  (0, 0, 0) when no probes are set.  Collective when nranks > 1:
        every rank calls it and receives the same bytes."""
        nv, cap = getattr(self, "_probe_nv", 0), getattr(self, "_probe_cap", 0)
        cnt = C.c_int64(0)
        out = np.zeros((max(cap, 1), nv, nv), dtype=np.float64)          # one (collective) call
        self._check(self.lib.dcfm_get_probe_draws(self.h, _ptr(out), C.byref(cnt)))
        return out[:cnt.value].copy()

    # -- per-sample precision draws --------------------------------------------------
    def set_precision_probes(self, V, capacity=None):
        """Record ``V' Sigma(s)^-1 V`` and ``log det Sigma(s)`` for every saved sample s of later runs
        (dcfm_set_precision_probes): V is (p,) or (p, nv), 0 <= nv <= 32, in Sigmaout's permuted,
        standardised coordinates (every rank passes the same V); a (p, 0) block records the log
        determinant alone.  Up to ``capacity`` draws are held (default ``mcmc // thin``).  Calling it
        again replaces V and resets the count; ``set_precision_probes(None)`` turns the recording off and
        frees its buffers.  Independent of ``set_probes``: both may be on at once."""
        if V is None:
            self._check(self.lib.dcfm_set_precision_probes(self.h, None, 0, 0))
            self._prec_nv = self._prec_cap = 0
            return
        p = self.P * self.g
        V = np.asarray(V, dtype=np.float64)
        if V.ndim not in (1, 2) or V.shape[0] != p:
            raise ValueError(f"V must be (p,) or (p, nv) with p = {p}, got {V.shape}")
        V2 = _f64F(V.reshape(p, -1) if V.ndim == 1 else V)
        if capacity is None:
            capacity = int(self.cfg.mcmc) // int(self.cfg.thin)
        self._check(self.lib.dcfm_set_precision_probes(self.h, _ptr(V2) if V2.shape[1] else None, V2.shape[1],
                                                       int(capacity)))
        self._prec_nv = V2.shape[1] if int(capacity) > 0 else 0
        self._prec_cap = int(capacity)

    def precision_draws(self):
        """``(Q, logdet)``: Q of shape (S, nv, nv) with ``Q[s] = V' Sigma(s)^-1 V`` in saved-sample order, every
        slice symmetric bit for bit, and logdet of shape (S,) with ``log det Sigma(s)``, Sigma(s) the
        per-sample matrix of dc:182-192.  Shapes (0, 0, 0) and (0,) when nothing is set.  Collective when
        nranks > 1: every rank calls it and receives the same bytes."""
        nv, cap = getattr(self, "_prec_nv", 0), getattr(self, "_prec_cap", 0)
        cnt = C.c_int64(0)
        Q = np.zeros((max(cap, 1), nv, nv), dtype=np.float64)           # one (collective) call
        ld = np.zeros(max(cap, 1), dtype=np.float64)
        self._check(self.lib.dcfm_get_precision_draws(self.h, _ptr(Q), _ptr(ld), C.byref(cnt)))
        return Q[:cnt.value].copy(), ld[:cnt.value].copy()

    # -- pointwise log-likelihood draws ------------------------------------------------
    def set_loglik(self, capacity=None):
        """Record, for every saved sample s of later runs, ``y_i' Sigma(s)^-1 y_i`` of every row i of the
        standardised data the sweep holds and ``log det Sigma(s)`` (dcfm_set_loglik).  Up to ``capacity``
        draws are held (default ``mcmc // thin``); later saved samples are not recorded.  Calling it again
        resets the count; ``set_loglik(0)`` turns the recording off and frees its buffers.  Independent of
        ``set_probes`` and ``set_precision_probes``: all three may be on at once."""
        if capacity is None:
            capacity = int(self.cfg.mcmc) // int(self.cfg.thin)
        self._check(self.lib.dcfm_set_loglik(self.h, int(capacity)))
        self._ll_cap = int(capacity)

    def loglik_draws(self, parts=False):
        """``ll`` of shape (S, n): ``ll[s, i] = log N(y_i; 0, Sigma(s)) = -(p log 2 pi + logdet[s] + maha[s, i]) / 2``,
        the pointwise log-likelihood of training row i (Y's row order, standardised units) under saved sample
        s -- the input of ``diagnostics.waic``.  ``parts=True`` returns ``(ll, maha, logdet)`` with maha (S, n)
        and logdet (S,).  Shapes (0, n) and (0,) when nothing is recorded.  Collective when nranks > 1: every
        rank calls it and receives the same bytes."""
        cap = getattr(self, "_ll_cap", 0)
        cnt = C.c_int64(0)
        maha = np.zeros((max(cap, 1), self.n), dtype=np.float64)          # one (collective) call
        ld = np.zeros(max(cap, 1), dtype=np.float64)
        self._check(self.lib.dcfm_get_loglik(self.h, _ptr(maha), _ptr(ld), C.byref(cnt)))
        maha, ld = maha[:cnt.value].copy(), ld[:cnt.value].copy()
        ll = -0.5 * (self.P * self.g * np.log(2.0 * np.pi) + ld[:, None] + maha)
        return (ll, maha, ld) if parts else ll

    # -- conditional prediction of unobserved variables --------------------------------
    def set_predict(self, Ynew, observed, capacity=None):
        """Predict the unobserved variables of new rows from their observed ones under every saved sample of
        later runs (dcfm_set_predict).  ``Ynew`` is (p,) or (p, nt), 0 <= nt <= 32 new rows as columns, in
        Sigmaout's permuted, standardised coordinates; ``observed`` is a (p,) mask, nonzero = observed, one
        mask for all rows; entries of Ynew at unobserved positions are ignored (NaN included).  ``Ynew=None``
        (or a (p, 0) block) accumulates the conditional variance and log det Sigma_AA(s) alone.  Up to
        ``capacity`` samples are accumulated (default ``mcmc // thin``); later saved samples are ignored.
        Calling it again replaces the inputs and zeroes the accumulators; ``set_predict(None, None, 0)``
        turns it off and frees its buffers.  One rank only: a sampler with a communicator raises
        DcfmError (DCFM_ERR_UNSUPPORTED).  Independent of the probes, precision probes and log-likelihood."""
        p = self.P * self.g
        if capacity is None:
            capacity = int(self.cfg.mcmc) // int(self.cfg.thin)
        if observed is None:
            if int(capacity) != 0:
                raise ValueError("observed is required unless capacity == 0")
            self._check(self.lib.dcfm_set_predict(self.h, None, None, 0, 0))
            self._pred_nt = self._pred_cap = 0
            return
        obs = np.ascontiguousarray(np.asarray(observed) != 0, dtype=np.uint8)
        if obs.shape != (p,):
            raise ValueError(f"observed must be ({p},), got {obs.shape}")
        Y = np.zeros((p, 0)) if Ynew is None else np.asarray(Ynew, dtype=np.float64)
        if Y.ndim not in (1, 2) or Y.shape[0] != p:
            raise ValueError(f"Ynew must be (p,) or (p, nt) with p = {p}, got {Y.shape}")
        Y2 = _f64F(Y.reshape(p, -1) if Y.ndim == 1 else Y)
        self._check(self.lib.dcfm_set_predict(self.h, _ptr(Y2) if Y2.shape[1] else None,
                                              obs.ctypes.data_as(C.POINTER(C.c_uint8)), Y2.shape[1], int(capacity)))
        self._pred_nt = Y2.shape[1] if int(capacity) > 0 else 0
        self._pred_cap = int(capacity)

    def predict_raw(self):
        """``(mean, m2, cvar, maha, logdet, count)`` exactly as dcfm_get_predict returns them: mean and m2
        (p, nt), cvar (p,), maha (count, nt), logdet (count,)."""
        nt, cap = getattr(self, "_pred_nt", 0), getattr(self, "_pred_cap", 0)
        p = self.P * self.g
        cnt = C.c_int64(0)
        mean = np.zeros((p, nt), dtype=np.float64, order="F")
        m2 = np.zeros((p, nt), dtype=np.float64, order="F")
        cvar = np.zeros(p, dtype=np.float64)
        maha = np.zeros((max(cap, 1), nt), dtype=np.float64)
        ld = np.zeros(max(cap, 1), dtype=np.float64)
        self._check(self.lib.dcfm_get_predict(self.h, _ptr(mean), _ptr(m2), _ptr(cvar), _ptr(maha), _ptr(ld),
                                              C.byref(cnt)))
        S = int(cnt.value)
        return mean, m2, cvar, maha[:S].copy(), ld[:S].copy(), S

    def predict(self) -> dict:
        """The conditional prediction accumulated so far, in standardised, permuted coordinates: ``mean``
        (p, nt) = avg_s E[y_j | y_A, Sigma(s)] (on an observed row: of the noise-free signal), ``sd_between``
        (p, nt) the standard deviation of that conditional mean over the samples, ``cvar`` (p,) = avg_s
        Var[y_j | y_A, Sigma(s)], ``sd_total`` (p, nt) = sqrt(cvar + var_between) (the law of total
        variance; the between-sample variance m2 - mean^2 clamped at 0), ``maha`` (count, nt) =
        y_A' Sigma_AA(s)^-1 y_A and ``logdet`` (count,) = log det Sigma_AA(s) per sample (the input of
        ``diagnostics.conditional_log_density``), and ``count``, the samples accumulated (the divisor).
        count 0 and empty draws when nothing is set or nothing was saved yet."""
        mean, m2, cvar, maha, ld, S = self.predict_raw()
        vb = np.maximum(m2 - mean * mean, 0.0)
        return {"mean": mean, "sd_between": np.sqrt(vb), "cvar": cvar, "sd_total": np.sqrt(cvar[:, None] + vb),
                "maha": maha, "logdet": ld, "count": S}

    # -- regression of a few variables on all the others ---------------------------------
    def set_regression(self, responses):
        """Accumulate, from the next run on, the posterior moments of the coefficients of the regression of the
        variables ``responses`` (up to 32 distinct 0-based indices in Sigmaout's permuted, standardised
        coordinates) on all the others (dcfm_set_regression; needs ``Sampler(..., regression=True)``).  Calling it
        again replaces the set and zeroes the accumulators; ``None`` or an empty list turns it off.  Every rank
        passes the same set."""
        r = np.ascontiguousarray(np.asarray([] if responses is None else responses, dtype=np.int64).reshape(-1))
        self._check(self.lib.dcfm_set_regression(
            self.h, r.ctypes.data_as(C.POINTER(C.c_int64)) if r.size else None, int(r.size)))
        self._reg_q, self._reg_resp = int(r.size), r.copy()

    def regression_raw(self):
        """``(coef, coef_m2, rcov, rcov_m2, r2, r2_m2, count)`` exactly as dcfm_get_regression returns them: coef
        and coef_m2 (p, q), rcov and rcov_m2 (q, q), r2 and r2_m2 (q,); all zeros with count 0."""
        q, p = getattr(self, "_reg_q", 0), self.P * self.g
        cnt = C.c_int64(0)
        coef, coef2 = (np.zeros((p, q), dtype=np.float64, order="F") for _ in range(2))
        rcov, rcov2 = (np.zeros((q, q), dtype=np.float64, order="F") for _ in range(2))
        r2, r22 = np.zeros(q, dtype=np.float64), np.zeros(q, dtype=np.float64)
        self._check(self.lib.dcfm_get_regression(self.h, _ptr(coef), _ptr(coef2), _ptr(rcov), _ptr(rcov2), _ptr(r2),
                                                 _ptr(r22), C.byref(cnt)))
        return coef, coef2, rcov, rcov2, r2, r22, int(cnt.value)

    def regression(self) -> dict:
        """The regression accumulated so far, in standardised, permuted coordinates: ``coef`` (p, q) the posterior
        mean of B(s) = Sigma_OO(s)^-1 Sigma_OR(s) (rows of the responses exactly 0: E[y_R | y_O] = coef' y),
        ``coef_sd`` its per-coefficient posterior SD, ``resid_cov`` / ``resid_cov_sd`` (q, q) those of the residual
        covariance Cov[y_R | y_O, Sigma(s)], ``r2`` / ``r2_sd`` (q,) those of 1 - C_jj / Sigma_jj, and ``count``, the
        samples accumulated (the divisor).  Each SD is sqrt(max(0, m2 - mean^2)).  ``responses`` repeats the set."""
        coef, coef2, rcov, rcov2, r2, r22, S = self.regression_raw()

        def sd(m, m2):
            return np.sqrt(np.maximum(m2 - m * m, 0.0))
        return {"coef": coef, "coef_sd": sd(coef, coef2), "resid_cov": rcov, "resid_cov_sd": sd(rcov, rcov2),
                "r2": r2, "r2_sd": sd(r2, r22), "count": S,
                "responses": getattr(self, "_reg_resp", np.zeros(0, dtype=np.int64)).copy()}

    # -- missing training data -----------------------------------------------------------
    def set_missing(self, mask, capacity=None):
        """Treat entries of the training data as missing (dcfm_set_missing): ``mask`` is (n, P, g_local) in
        ``Yd_local``'s layout, nonzero = missing.  From the next run on, every iteration ends with a
        data-augmentation step that redraws the missing entries of the device's Y from
        ``N(eta_i . lambda_j, 1 / ps_j)`` and refreshes the columns' sums of squares, so the sweep runs on the
        completed matrix (``get_data()`` reads the current draw).  Call it after ``set_data`` / ``set_data_raw``; a
        later ``set_data*`` turns it off.  A missing entry whose uploaded value is finite starts there, a NaN one at
        0.  Up to ``capacity`` saved samples are accumulated for ``imputed()`` (default ``mcmc // thin``; 0 = draw
        only).  Calling it again replaces the mask and zeroes the accumulators; ``None`` or an all-False mask turns
        the feature off.  Every rank passes the mask of its own shards.  Not together with ``set_loglik``
        (DcfmError, DCFM_ERR_UNSUPPORTED, in either order)."""
        if capacity is None:
            capacity = int(self.cfg.mcmc) // int(self.cfg.thin)
        if mask is None:
            self._check(self.lib.dcfm_set_missing(self.h, None, int(capacity)))
            self._miss_mask = None
            return
        mk = np.asfortranarray(np.asarray(mask) != 0, dtype=np.uint8)
        if mk.shape != (self.n, self.P, self.g_local):
            raise ValueError(f"mask must be n x P x g_local = {(self.n, self.P, self.g_local)}, got {mk.shape}")
        self._check(self.lib.dcfm_set_missing(self.h, mk.ctypes.data_as(C.POINTER(C.c_uint8)), int(capacity)))
        self._miss_mask = mk.astype(bool) if mk.any() else None

    def imputed_raw(self):
        """``(mean, m2, nvar, count)`` exactly as dcfm_get_imputed returns them: mean and m2 (n, P, g_local),
        nvar (P, g_local); all zeros while count is 0."""
        cnt = C.c_int64(0)
        mean = np.zeros((self.n, self.P, self.g_local), dtype=np.float64, order="F")
        m2 = np.zeros((self.n, self.P, self.g_local), dtype=np.float64, order="F")
        nvar = np.zeros((self.P, self.g_local), dtype=np.float64, order="F")
        self._check(self.lib.dcfm_get_imputed(self.h, _ptr(mean), _ptr(m2), _ptr(nvar), C.byref(cnt)))
        return mean, m2, nvar, int(cnt.value)

    def imputed(self) -> dict:
        """The imputation accumulated so far, in ``Yd_local``'s layout and standardised units: ``mean`` (n, P,
        g_local) = the posterior mean of ``eta_i . lambda_j`` at a missing entry and the data at an observed one,
        ``sd_between`` the standard deviation of that conditional mean over the samples, ``sd_total`` =
        sqrt(avg_s 1 / ps_j + var_between) the total predictive standard deviation (the law of total variance; the
        between-sample variance m2 - mean^2 clamped at 0), both 0 at observed entries, ``count`` the samples
        accumulated (the divisor) and ``mask`` the boolean mask in force.  count 0 (and zeros) when nothing is
        set, the capacity is 0 or nothing was saved yet."""
        mean, m2, nvar, S = self.imputed_raw()
        mk = getattr(self, "_miss_mask", None)
        if mk is None:
            mk = np.zeros(mean.shape, dtype=bool)
        vb = np.where(mk, np.maximum(m2 - mean * mean, 0.0), 0.0)
        tot = np.where(mk, nvar[None, :, :] + vb, 0.0) if S else np.zeros(mean.shape)
        return {"mean": mean, "sd_between": np.sqrt(vb), "sd_total": np.sqrt(tot), "count": S, "mask": mk}

    # -- measurement -----------------------------------------------------------------
    def set_profiling(self, on: bool):
        self._check(self.lib.dcfm_set_profiling(self.h, 1 if on else 0))

    def set_profiling_kernels(self, names, stride: int = 1):
        """Time only these kernels (names of _abi.KERNEL_IDS); empty = off.  stride > 1 times
        one in `stride` launches of each (the event records cost device time per launch)."""
        mask = 0
        for nm in names:
            mask |= 1 << _abi.KERNEL_IDS[nm]
        self._check(self.lib.dcfm_set_profiling_mask(self.h, mask))
        if stride != 1:
            self._check(self.lib.dcfm_set_profiling_stride(self.h, int(stride)))

    def kernel_stats(self) -> dict:
        ms = (C.c_double * _abi.K_COUNT)()
        cnt = (C.c_int64 * _abi.K_COUNT)()
        self._check(self.lib.dcfm_get_kernel_stats(self.h, ms, cnt))
        return {name: (ms[i], cnt[i]) for name, i in _abi.KERNEL_IDS.items()}


def count_nonzero_columns(Y, device=0, return_ms=False):
    """dc:31-34 on the device: nnz of every column of the n x p matrix Y (int32)."""
    lib = _abi.load_library()
    Y = _f64F(Y)
    if Y.ndim != 2:
        raise ValueError("Y must be n x p")
    out = np.zeros(Y.shape[1], dtype=np.int32)
    ms = C.c_double(0.0)
    rc = lib.dcfm_count_nonzero_columns(int(device), _ptr(Y), Y.shape[0], Y.shape[1],
                                        out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ms))
    _abi.check(lib, None, rc)
    return (out, ms.value) if return_ms else out


def rng_fill(kind: str, count: int, *, seed=0, shape=1.0, site=15, shard=0, iteration=0, device=0, width=32):
    """On-device Philox variates exactly as the sweep draws them (diagnostic): variate e at the
    counter (site, shard, row = e // width, index = e % width, iteration)."""
    lib = _abi.load_library()
    out = np.zeros(int(count), dtype=np.float64)
    k = {"normal": 0, "gamma": 1}[kind]
    if width == 32:
        rc = lib.dcfm_rng_fill(int(device), int(seed), k, float(shape), int(site), int(shard),
                               int(iteration), int(count), _ptr(out))
    else:
        rows = (int(count) + int(width) - 1) // int(width)
        rc = lib.dcfm_rng_fill_rows(int(device), int(seed), k, float(shape), int(site), int(shard),
                                    int(iteration), rows, int(width), int(count), _ptr(out))
    _abi.check(lib, None, rc)
    return out
