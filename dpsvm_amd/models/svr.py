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

import time
from typing import Any, Callable, Optional

import numpy as np

from .._native import load
from ._base import _OneBlockEstimator, _as_1d, _train_input
from .svc import LoadedModel


def _r2(z, pred: np.ndarray) -> float:
    """the coefficient of determination R^2 = 1 - sum (z - pred)^2 / sum (z - mean z)^2 (float64)"""
    z = np.asarray(_as_1d(z), dtype=np.float64)
    r = z - pred.astype(np.float64)
    den = float(np.sum((z - z.mean()) ** 2))
    return 1.0 - float(np.sum(r * r)) / den if den > 0 else 0.0


class SVR(_OneBlockEstimator):
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

    _NAME, _KIND, _EXTRA = "SVR", "regression", "epsilon"
    _RUNS = "epsilon-SVR runs one-block working-set rounds on the resident Gram of one rank, with box clipping"
    _CLIP_WHY = "a pair (j, j + n) has eta = 0: only the joint box removes its common part"

    def __init__(self, C: float = 1.0, gamma: Optional[float] = None, epsilon: float = 0.1, eps: float = 1e-3,
                 max_iter: int = 150000, device: str = "auto", **kwargs: Any):
        self.epsilon = float(epsilon)
        super().__init__(C=C, gamma=gamma, eps=eps, max_iter=max_iter, device=device, **kwargs)

    def _check_extra(self) -> None:
        if not (self.epsilon >= 0.0 and np.isfinite(self.epsilon)):
            raise ValueError(f"epsilon must be >= 0, got {self.epsilon}")

    def _params(self, d: int):
        p = self.config.to_native(d)
        p.problem = 1
        p.svr_epsilon = self.epsilon
        return p

    def fit(self, X, z, comm=None, resume=None, progress: Optional[Callable] = None, rank_rows=None,
            sample_weight=None) -> "SVR":
        """Train on real-valued targets ``z``.  One rank, from a cold start, unweighted."""
        self._refuse_fit_args(comm, resume, rank_rows, sample_weight)
        self._resolve()
        # kernel="precomputed": X is the (n, n) Gram; predict() then takes K(test, train).  A kernel spec: the rows
        X = _train_input(self.config, X)
        z = np.ascontiguousarray(_as_1d(z), dtype=np.float32)
        n, d = X.shape
        if z.shape[0] != n:
            raise ValueError("len(z) != X.shape[0]")
        if not np.all(np.isfinite(z)):
            raise ValueError("targets must be finite")
        p = self._params(d)
        t0 = time.perf_counter()
        alpha, info, _, setup = self._run(X, z, p, progress, want_gradient=False)
        self.wall_time_ = time.perf_counter() - t0
        raw = np.asarray(alpha, dtype=np.float32).reshape(2, n)
        # the canonical dual pair: the common part min(alpha_j, alpha*_j) removed.  It leaves beta, the equality
        # constraint and the box as they are and never raises the objective (it lowers it by 2 epsilon per
        # unit), and the stop test cannot see it once 2 epsilon <= 2 eps: the pair (j, j + n) violates by exactly
        # 2 epsilon — at epsilon = 0 the objective is flat along it and the solver has no reason to remove it
        common = np.minimum(raw[0], raw[1])
        self.alpha_ = np.ascontiguousarray(raw - common[None, :])
        self.n_common_ = int(np.sum(common > 0))
        self._publish_fit(X, self.alpha_[0] - self.alpha_[1], info, p.gamma, setup)
        return self

    def predict(self, X, predict_chunk_rows=None) -> np.ndarray:
        """sum_sv beta K(sv, x) - b, float32 (``predict_chunk_rows``: a kernel spec's test rows per chunk)"""
        return self._decision(X, predict_chunk_rows=predict_chunk_rows)

    def score(self, X, z, predict_chunk_rows=None) -> float:
        """R^2 of the predictions"""
        return _r2(z, self.predict(X, predict_chunk_rows))


class LoadedSVR(LoadedModel):
    """A regression model read from the binary text model file: ``predict`` is the decision value."""

    predict = LoadedModel.decision_function

    def score(self, X, z, predict_chunk_rows=None) -> float:
        return _r2(z, self.predict(X, predict_chunk_rows))


def load_svr(path: str, device: str = "auto") -> LoadedSVR:
    """The regression predictor of a model file written by ``SVR.save``."""
    return LoadedSVR(load().read_model(path, False), device)
