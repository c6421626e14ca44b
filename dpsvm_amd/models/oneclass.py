"""OneClassSVM: novelty detection (LIBSVM ``-s 2``) on the classifier's machinery.

The dual of the one-class SVM is ``min 1/2 a'Ka`` subject to ``0 <= a_i <= 1`` and
``sum a = nu n``.  With every label +1 the classifier's working-set rounds, its stop
test ``!(b_lo > b_hi + 2 eps)`` and ``b = (b_hi + b_lo) / 2`` (here rho) solve it as
they stand; what differs is the start.  ``a = 0`` is infeasible, so the solve begins
at LIBSVM's point — 1 on the first floor(nu n) rows, the remainder on the next — with
``f = K a`` read off the resident Gram by one memory-bound kernel that accumulates in
fp64 (gram_rows_wsum, docs/DESIGN.md §18).  nu changes only that start: a sweep over
nu is k solves on one setup and one Gram (``nu_path``).

The model ``sum_i a_i K(x_i, x) - rho`` is a binary model with y = +1: the predictors
and the text model format serve unchanged.

scikit-learn names: ``offset_`` is rho, ``eps`` stays this project's stop tolerance
(scikit-learn's ``tol``).
"""
from __future__ import annotations

import dataclasses
import time
from typing import Any, Callable, Optional, Sequence

import numpy as np

from .._native import load
from .svc import SVCConfig, _as_f32_2d, _parse_device

# what one-class runs on: one-block working-set rounds on the resident Gram, one rank, joint-box clipping
_NOTE = "one-class: nu start, one block"


def _refuse(what: str) -> None:
    raise NotImplementedError(f"OneClassSVM: {what} is not implemented for one-class (it runs one-block "
                              "working-set rounds on the resident Gram of one rank, with box clipping and C = 1)")


def _check_nu(nu: float) -> float:
    nu = float(nu)
    if not (0.0 < nu < 1.0):
        raise ValueError(f"nu must lie in (0, 1), got {nu}")
    return nu


class OneClassSVM:
    """RBF one-class SVM: ``min 1/2 |w|^2 - rho + 1/(nu n) sum max(0, rho - w.phi(x_i))``.

    Attributes after ``fit(X)``: ``alpha_`` ((n,), LIBSVM's scale: 0 <= alpha <= 1, sum = nu n), ``dual_coef_``
    (alpha of the support vectors), ``support_``, ``support_vectors_``, ``n_support_``, ``offset_`` (= rho =
    ``b_``), ``intercept_`` (= -rho), ``train_decision_`` (f - rho of the training rows, from the solver's
    gradient: no predict pass), ``n_iter_``, ``n_rounds_``, ``status_``, ``converged_``, ``fit_time_``,
    ``stats_`` and ``setup_info_``.

    The settings resolve to ``solver="ws"``, ``ws_blocks=1``, ``clip="box"``, ``shrink="off"``,
    ``ws_recompute="off"``; asking for anything else raises.  Independent clipping would let sum(alpha) drift
    from nu n, so the joint box only.  nu = 1 (every alpha at its bound: nothing to solve) is refused.
    """

    def __init__(self, nu: float = 0.5, gamma: Optional[float] = None, eps: float = 1e-3, max_iter: int = 150000,
                 device: str = "auto", **kwargs: Any):
        kwargs.setdefault("clip", "box")
        if kwargs.get("C", 1.0) != 1.0:
            _refuse(f"C={kwargs['C']} (the box is [0, 1])")
        kwargs.pop("C", None)
        self.config = SVCConfig(C=1.0, gamma=gamma, eps=eps, max_iter=max_iter, device=device, **kwargs)
        self.nu = nu
        self._resolve()
        self._model = None
        self._gpu_pred = None

    # ------------------------------------------------------------------ settings
    def _resolve(self) -> None:
        """refuse what one-class does not run, resolve the rest (before any native or device state exists)"""
        cfg = self.config
        self.nu = _check_nu(self.nu)
        _parse_device(cfg.device)
        if cfg.C != 1.0:
            _refuse(f"C={cfg.C} (the box is [0, 1])")
        if cfg.clip != "box":
            _refuse(f"clip={cfg.clip!r} (independent clipping lets sum(alpha) drift from nu n)")
        if cfg.solver not in ("auto", "ws"):
            _refuse(f"solver={cfg.solver!r} (the pair-at-a-time engines)")
        if cfg.ws_blocks not in (0, 1):
            _refuse(f"ws_blocks={cfg.ws_blocks} (multi-block rounds)")
        if cfg.shrink_mode() == "on":
            _refuse("shrink='on'")
        if cfg.ws_recompute == "on":
            _refuse("ws_recompute='on'")
        if cfg.class_weight is not None:
            _refuse("class_weight (per-row C)")
        if cfg.force_cache or cfg.cache_lines or cfg.host_cache_lines:
            _refuse("the kernel-row cache (force_cache / cache_lines / host_cache_lines)")
        if cfg.engines != "production":
            _refuse("engines='all'")
        if cfg.x_mode == "partitioned" or cfg.dp != "auto":
            _refuse("partitioned X / a data-parallel policy")
        if cfg.exchange == "peer" or cfg.force_collectives:
            _refuse("the peer exchange / forced collectives")
        if cfg.checkpoint_path or cfg.checkpoint_every:
            _refuse("checkpoints")
        cfg.solver = "ws"
        cfg.ws_blocks = 1
        cfg.shrink = "off"
        cfg.ws_recompute = "off"

    def _params(self, d: int, nu: Optional[float] = None):
        p = self.config.to_native(d)
        p.one_class_nu = self.nu if nu is None else nu
        return p

    @staticmethod
    def _refuse_fit_args(comm, resume, rank_rows, sample_weight) -> None:
        for name, val in (("comm", comm), ("resume", resume), ("rank_rows", rank_rows),
                          ("sample_weight", sample_weight)):
            if val is not None:
                _refuse(name)

    # ------------------------------------------------------------------ fit
    def fit(self, X, y=None, comm=None, resume=None, progress: Optional[Callable] = None, rank_rows=None,
            sample_weight=None) -> "OneClassSVM":
        """Train on the rows of ``X`` (``y`` is ignored).  One rank, from the nu start, unweighted."""
        self._refuse_fit_args(comm, resume, rank_rows, sample_weight)
        self._resolve()
        X = _as_f32_2d(X)
        n, d = X.shape
        C = load()
        p = self._params(d)
        ones = np.ones(n, dtype=np.float32)
        kind, dev = self.config.device_kind()
        t0 = time.perf_counter()
        if kind == "cuda":
            solver = C.GpuSolver(p, None, dev)  # dropped after the solve, with its resident Gram
            self.setup_info_ = solver.setup(X, n, ones)
            alpha, info = solver.solve(None, progress)
            f = np.asarray(solver.gradient(), dtype=np.float32)
            del solver
            info = dict(info)
        else:
            self.setup_info_ = {"iteration": "cpu", "engine_note": _NOTE}
            alpha, info = C.solve_cpu(X, ones, p, None, None, progress, None)
            info = dict(info)
            f = np.asarray(info.pop("f"), dtype=np.float32)
        self.wall_time_ = time.perf_counter() - t0
        self._publish(X, alpha, info, f, p.gamma)
        self.device_ = f"{kind}:{dev}" if kind == "cuda" else "cpu"
        return self

    def _publish(self, X: np.ndarray, alpha: np.ndarray, info: dict, f: np.ndarray, gamma: float) -> None:
        n, d = X.shape
        self.alpha_ = np.ascontiguousarray(np.asarray(alpha, dtype=np.float32).reshape(n))
        self.b_ = float(info["b"])
        self.offset_ = self.b_
        self.intercept_ = -self.b_
        self.train_decision_ = (f.astype(np.float64) - self.b_).astype(np.float32)
        self.n_iter_ = int(info["iters"])
        self.n_rounds_ = int(info.get("outer", 0))
        self.status_ = int(info["status"])
        self.converged_ = bool(info["converged"])
        self.fit_time_ = float(info["t_solve"])
        self.setup_time_ = float(info["t_setup"])
        self.stats_ = info
        self.gamma_ = gamma
        self.n_features_in_ = d
        self.support_ = np.nonzero(self.alpha_ > 0)[0]
        self.support_vectors_ = X[self.support_]
        self.dual_coef_ = self.alpha_[self.support_].astype(np.float32)
        self.n_support_ = int(len(self.support_))
        self._X_train = X
        self._model = None
        self._gpu_pred = None
        if self.status_ == 2:
            import warnings

            warnings.warn(f"stopped at max_iter with gap {info['b_lo'] - info['b_hi']:.3g} > 2 eps: raise max_iter "
                          "to converge", RuntimeWarning, stacklevel=3)

    def nu_path(self, X, nus: Sequence[float], progress: Optional[Callable] = None) -> dict:
        """One solve per nu on one solver, one ``setup()`` and one resident Gram (``set_nu`` per nu; on the CPU k
        plain solves).  Returns ``{"nu", "rho", "n_support", "outlier_fraction"}`` (the fraction of training rows
        with a negative decision) and keeps ``path_stats_`` (the solves' info dicts: ``gram_reused`` reads
        [False, True, ...]) and ``path_alpha_`` ((k, n)).  The estimator's own fit is left as it is."""
        self._resolve()
        nus = [_check_nu(v) for v in nus]
        if not nus:
            raise ValueError("nu_path needs at least one nu")
        X = _as_f32_2d(X)
        n, d = X.shape
        C = load()
        ones = np.ones(n, dtype=np.float32)
        kind, dev = self.config.device_kind()
        rho, nsv, out, stats, alphas = [], [], [], [], []
        solver = None
        if kind == "cuda":
            solver = C.GpuSolver(self._params(d, nus[0]), None, dev)
            self.path_setup_info_ = solver.setup(X, n, ones)
        for i, nu in enumerate(nus):
            if solver is not None:
                if i > 0:
                    solver.set_nu(nu)
                alpha, info = solver.solve(None, progress)
                info = dict(info)
                f = np.asarray(solver.gradient(), dtype=np.float64)
            else:
                alpha, info = C.solve_cpu(X, ones, self._params(d, nu), None, None, progress, None)
                info = dict(info)
                f = np.asarray(info.pop("f"), dtype=np.float64)
            alpha = np.asarray(alpha, dtype=np.float32)
            rho.append(float(info["b"]))
            nsv.append(int(np.count_nonzero(alpha > 0)))
            out.append(float(np.mean(f - float(info["b"]) < 0)))
            stats.append(info)
            alphas.append(alpha)
        del solver
        self.path_stats_ = stats
        self.path_alpha_ = np.stack(alphas)
        return {"nu": list(nus), "rho": rho, "n_support": nsv, "outlier_fraction": out}

    # ------------------------------------------------------------------ model
    def to_model(self):
        """the binary model of alpha with y = +1 (rows with alpha = 0 are no SVs), b = rho"""
        if self._model is None:
            if getattr(self, "alpha_", None) is None:
                raise RuntimeError("to_model() needs a fitted OneClassSVM")
            y = np.ones(len(self.alpha_), dtype=np.float32)
            self._model = load().make_model(self._X_train, y, self.alpha_, self.b_, self.gamma_)
        return self._model

    def save(self, path: str, precision: int = 9) -> None:
        """Write the binary text model (gamma, rho, then alpha, +1, x per SV); ``load_one_class`` reads it."""
        load().write_model(path, self.to_model(), precision, False)

    # ------------------------------------------------------------------ predict
    def _predictor(self):
        if self._gpu_pred is None:
            kind, dev = self.config.device_kind()
            if kind == "cuda":
                self._gpu_pred = load().GpuPredictor(self.to_model(), dev)
        return self._gpu_pred

    def decision_function(self, X) -> np.ndarray:
        """sum_sv alpha K(sv, x) - rho, float32: >= 0 inside the estimated support"""
        X = _as_f32_2d(X)
        if X.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {X.shape[1]} features, model has {self.n_features_in_}")
        gp = self._predictor()
        out = gp.decision(X) if gp is not None else load().decision_cpu(self.to_model(), X, 0)
        return np.asarray(out, dtype=np.float32)

    def score_samples(self, X) -> np.ndarray:
        """the decision without the offset: sum_sv alpha K(sv, x)"""
        return (self.decision_function(X) + np.float32(self.offset_)).astype(np.float32)

    def predict(self, X) -> np.ndarray:
        """+1 where the decision is >= 0 (inlier), else -1"""
        return np.where(self.decision_function(X) >= 0, 1, -1).astype(np.int32)

    def get_params(self, deep: bool = True) -> dict:
        out = dataclasses.asdict(self.config)
        out["nu"] = self.nu
        return out


class LoadedOneClass:
    """A one-class model read from the binary text model file."""

    def __init__(self, model, device: str = "auto"):
        self.model = model
        self.device = device
        if device != "auto":
            _parse_device(device)
        self._gpu = None

    @property
    def gamma(self) -> float:
        return self.model.gamma

    @property
    def offset(self) -> float:
        return self.model.b

    @property
    def n_support(self) -> int:
        return self.model.nsv

    def _predictor(self):
        kind, dev = _parse_device(self.device)
        if kind == "cuda" and self._gpu is None:
            self._gpu = load().GpuPredictor(self.model, dev)
        return self._gpu

    def decision_function(self, X) -> np.ndarray:
        X = _as_f32_2d(X)
        gp = self._predictor()
        out = gp.decision(X) if gp is not None else load().decision_cpu(self.model, X, 0)
        return np.asarray(out, dtype=np.float32)

    def score_samples(self, X) -> np.ndarray:
        return (self.decision_function(X) + np.float32(self.offset)).astype(np.float32)

    def predict(self, X) -> np.ndarray:
        return np.where(self.decision_function(X) >= 0, 1, -1).astype(np.int32)


def load_one_class(path: str, device: str = "auto") -> LoadedOneClass:
    """The one-class predictor of a model file written by ``OneClassSVM.save``."""
    return LoadedOneClass(load().read_model(path, False), device)
