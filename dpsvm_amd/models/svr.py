"""SVR: epsilon-insensitive support vector regression on the classifier's machinery.

The dual of epsilon-SVR has 2n variables — alpha_j (label +1) and alpha*_j (label -1)
per training row — whose kernel matrix is the n x n Gram tiled 2 x 2, and a linear
term [eps - z, eps + z] instead of the classifier's -1.  The solvers run that dual
*folded*: kernel rows, the resident Gram, X and |x|^2 stay n-sized, only the state
(alpha, f, the labels) has 2n rows; the f update reads each Gram value once for both
halves (docs/DESIGN.md §17).  Everything else — the I_up / I_low sets, the stop test
``!(b_lo > b_hi + 2 eps)``, ``b = (b_hi + b_lo) / 2``, the pair rule — is the
classifier's.  The result beta = alpha - alpha* is a binary model with alpha = |beta|,
y = sign(beta): the predictors and the text model format serve unchanged, and a
prediction is the decision value sum_i beta_i K(x_i, x) - b.

scikit-learn names: ``epsilon`` is the tube's half width, ``eps`` stays this
project's stop tolerance (scikit-learn's ``tol``).
"""
from __future__ import annotations

import dataclasses
import time
from typing import Any, Callable, Optional

import numpy as np

from .._native import load
from .svc import SVCConfig, _as_1d, _as_f32_2d, _parse_device

# what regression runs on: one-block working-set rounds on the resident Gram, one rank, joint-box clipping
_NOTE = "epsilon-SVR: folded 2n, one block"


def _refuse(what: str) -> None:
    raise NotImplementedError(f"SVR: {what} is not implemented for regression (epsilon-SVR runs one-block "
                              "working-set rounds on the resident Gram of one rank, with box clipping)")


class SVR:
    """RBF epsilon-SVR: ``min 1/2 |w|^2 + C sum max(0, |z_i - f(x_i)| - epsilon)``.

    Attributes after fit: ``alpha_`` ((2, n): alpha and alpha*), ``dual_coef_`` (beta = alpha - alpha* of the
    support vectors), ``support_``, ``support_vectors_``, ``n_support_``, ``b_`` (prediction = sum beta_i
    K(x_i, x) - b), ``intercept_`` (= -b_), ``n_iter_``, ``n_rounds_``, ``status_``, ``converged_``,
    ``fit_time_``, ``stats_`` and (GPU) ``setup_info_``; ``n_common_`` counts the rows whose raw solver output
    had alpha_j and alpha*_j both positive (0 whenever epsilon > eps: the stop test sees such a pair).

    The settings resolve to ``solver="ws"``, ``ws_blocks=1``, ``clip="box"``, ``shrink="off"``,
    ``ws_recompute="off"``; asking for anything else raises.  A pair (j, j + n) of the folded dual has eta = 0
    and violates only while alpha_j and alpha*_j are both positive: the eta floor and the joint box then remove
    their common part, which independent clipping would not — hence box clipping only.
    """

    def __init__(self, C: float = 1.0, gamma: Optional[float] = None, epsilon: float = 0.1, eps: float = 1e-3,
                 max_iter: int = 150000, device: str = "auto", **kwargs: Any):
        kwargs.setdefault("clip", "box")
        self.config = SVCConfig(C=C, gamma=gamma, eps=eps, max_iter=max_iter, device=device, **kwargs)
        self.epsilon = float(epsilon)
        self._resolve()
        self._model = None
        self._gpu_pred = None

    # ------------------------------------------------------------------ settings
    def _resolve(self) -> None:
        """refuse what regression does not run, resolve the rest (before any native or device state exists)"""
        cfg = self.config
        if not (self.epsilon >= 0.0 and np.isfinite(self.epsilon)):
            raise ValueError(f"epsilon must be >= 0, got {self.epsilon}")
        _parse_device(cfg.device)
        if cfg.clip != "box":
            _refuse(f"clip={cfg.clip!r} (a pair (j, j + n) has eta = 0: only the joint box removes its common part)")
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

    def _params(self, d: int):
        p = self.config.to_native(d)
        p.problem = 1
        p.svr_epsilon = self.epsilon
        return p

    # ------------------------------------------------------------------ fit
    def fit(self, X, z, comm=None, resume=None, progress: Optional[Callable] = None, rank_rows=None,
            sample_weight=None) -> "SVR":
        """Train on real-valued targets ``z``.  One rank, from a cold start, unweighted."""
        for name, val in (("comm", comm), ("resume", resume), ("rank_rows", rank_rows),
                          ("sample_weight", sample_weight)):
            if val is not None:
                _refuse(name)
        self._resolve()
        X = _as_f32_2d(X)
        z = np.ascontiguousarray(_as_1d(z), dtype=np.float32)
        n, d = X.shape
        if z.shape[0] != n:
            raise ValueError("len(z) != X.shape[0]")
        if not np.all(np.isfinite(z)):
            raise ValueError("targets must be finite")
        C = load()
        p = self._params(d)
        kind, dev = self.config.device_kind()
        t0 = time.perf_counter()
        if kind == "cuda":
            solver = C.GpuSolver(p, None, dev)  # dropped after the solve, with its resident Gram
            self.setup_info_ = solver.setup(X, n, z)
            alpha, info = solver.solve(None, progress)
            del solver
        else:
            self.setup_info_ = {"iteration": "cpu", "engine_note": _NOTE}
            alpha, info = C.solve_cpu(X, z, p, None, None, progress, None)
        self.wall_time_ = time.perf_counter() - t0
        self._publish(X, alpha, dict(info), p.gamma)
        self.device_ = f"{kind}:{dev}" if kind == "cuda" else "cpu"
        return self

    def _publish(self, X: np.ndarray, alpha: np.ndarray, info: dict, gamma: float) -> None:
        n, d = X.shape
        raw = np.asarray(alpha, dtype=np.float32).reshape(2, n)
        # the canonical dual pair: the common part min(alpha_j, alpha*_j) removed.  It leaves beta, the equality
        # constraint and the box as they are and never raises the objective (it lowers it by 2 epsilon per
        # unit), and the stop test cannot see it once 2 epsilon <= 2 eps: the pair (j, j + n) violates by exactly
        # 2 epsilon — at epsilon = 0 the objective is flat along it and the solver has no reason to remove it
        common = np.minimum(raw[0], raw[1])
        self.alpha_ = np.ascontiguousarray(raw - common[None, :])
        self.n_common_ = int(np.sum(common > 0))
        beta = self.alpha_[0] - self.alpha_[1]
        self.b_ = float(info["b"])
        self.intercept_ = -self.b_
        self.n_iter_ = int(info["iters"])
        self.n_rounds_ = int(info.get("outer", 0))
        self.status_ = int(info["status"])
        self.converged_ = bool(info["converged"])
        self.fit_time_ = float(info["t_solve"])
        self.setup_time_ = float(info["t_setup"])
        self.stats_ = info
        self.gamma_ = gamma
        self.n_features_in_ = d
        self.support_ = np.nonzero(beta != 0)[0]
        self.support_vectors_ = X[self.support_]
        self.dual_coef_ = beta[self.support_].astype(np.float32)
        self.n_support_ = int(len(self.support_))
        self._X_train, self._beta = X, beta
        self._model = None
        self._gpu_pred = None
        if self.status_ == 2:
            import warnings

            warnings.warn(f"stopped at max_iter with gap {info['b_lo'] - info['b_hi']:.3g} > 2 eps: raise max_iter "
                          "to converge", RuntimeWarning, stacklevel=3)

    # ------------------------------------------------------------------ model
    def to_model(self):
        """the binary model of beta: alpha = |beta|, y = sign(beta) (rows with beta = 0 are no SVs)"""
        if self._model is None:
            if getattr(self, "_beta", None) is None:
                raise RuntimeError("to_model() needs a fitted SVR")
            y = np.where(self._beta < 0, -1.0, 1.0).astype(np.float32)
            self._model = load().make_model(self._X_train, y, np.abs(self._beta).astype(np.float32), self.b_,
                                            self.gamma_)
        return self._model

    def save(self, path: str, precision: int = 9) -> None:
        """Write the binary text model (gamma, b, then |beta|, sign(beta), x per SV); ``load_svr`` reads it."""
        load().write_model(path, self.to_model(), precision, False)

    # ------------------------------------------------------------------ predict
    def _predictor(self):
        if self._gpu_pred is None:
            kind, dev = self.config.device_kind()
            if kind == "cuda":
                self._gpu_pred = load().GpuPredictor(self.to_model(), dev)
        return self._gpu_pred

    def predict(self, X) -> np.ndarray:
        """sum_sv beta K(sv, x) - b, float32"""
        X = _as_f32_2d(X)
        if X.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {X.shape[1]} features, model has {self.n_features_in_}")
        gp = self._predictor()
        out = gp.decision(X) if gp is not None else load().decision_cpu(self.to_model(), X, 0)
        return np.asarray(out, dtype=np.float32)

    def score(self, X, z) -> float:
        """the coefficient of determination R^2 = 1 - sum (z - pred)^2 / sum (z - mean z)^2 (float64)"""
        z = np.asarray(_as_1d(z), dtype=np.float64)
        r = z - self.predict(X).astype(np.float64)
        den = float(np.sum((z - z.mean()) ** 2))
        return 1.0 - float(np.sum(r * r)) / den if den > 0 else 0.0

    def get_params(self, deep: bool = True) -> dict:
        out = dataclasses.asdict(self.config)
        out["epsilon"] = self.epsilon
        return out


class LoadedSVR:
    """A regression model read from the binary text model file: ``predict`` is the decision value."""

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
    def b(self) -> float:
        return self.model.b

    @property
    def n_support(self) -> int:
        return self.model.nsv

    def _predictor(self):
        kind, dev = _parse_device(self.device)
        if kind == "cuda" and self._gpu is None:
            self._gpu = load().GpuPredictor(self.model, dev)
        return self._gpu

    def predict(self, X) -> np.ndarray:
        X = _as_f32_2d(X)
        gp = self._predictor()
        out = gp.decision(X) if gp is not None else load().decision_cpu(self.model, X, 0)
        return np.asarray(out, dtype=np.float32)

    def score(self, X, z) -> float:
        z = np.asarray(_as_1d(z), dtype=np.float64)
        r = z - self.predict(X).astype(np.float64)
        den = float(np.sum((z - z.mean()) ** 2))
        return 1.0 - float(np.sum(r * r)) / den if den > 0 else 0.0


def load_svr(path: str, device: str = "auto") -> LoadedSVR:
    """The regression predictor of a model file written by ``SVR.save``."""
    return LoadedSVR(load().read_model(path, False), device)
