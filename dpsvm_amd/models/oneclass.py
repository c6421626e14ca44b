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

import time
from typing import Any, Callable, Optional, Sequence

import numpy as np

from .._native import load
from ._base import _OneBlockEstimator, _train_input
from .svc import LoadedModel


def _check_nu(nu: float) -> float:
    nu = float(nu)
    if not (0.0 < nu < 1.0):
        raise ValueError(f"nu must lie in (0, 1), got {nu}")
    return nu


class _OneClassDecisions:
    """what the estimator and the loaded model derive from the decision sum_sv alpha K(sv, x) - rho"""

    def decision_function(self, X, predict_chunk_rows=None) -> np.ndarray:
        """float32: >= 0 inside the estimated support (``predict_chunk_rows``: a kernel spec's test rows per chunk)"""
        return self._decision(X, predict_chunk_rows=predict_chunk_rows)

    def score_samples(self, X, predict_chunk_rows=None) -> np.ndarray:
        """the decision without the offset: sum_sv alpha K(sv, x)"""
        return (self.decision_function(X, predict_chunk_rows) + np.float32(self._rho())).astype(np.float32)

    def predict(self, X, predict_chunk_rows=None) -> np.ndarray:
        """+1 where the decision is >= 0 (inlier), else -1"""
        return np.where(self.decision_function(X, predict_chunk_rows) >= 0, 1, -1).astype(np.int32)


class OneClassSVM(_OneClassDecisions, _OneBlockEstimator):
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

    _NAME, _KIND, _EXTRA = "OneClassSVM", "one-class", "nu"
    _RUNS = "it runs one-block working-set rounds on the resident Gram of one rank, with box clipping and C = 1"
    _CLIP_WHY = "independent clipping lets sum(alpha) drift from nu n"

    def __init__(self, nu: float = 0.5, gamma: Optional[float] = None, eps: float = 1e-3, max_iter: int = 150000,
                 device: str = "auto", **kwargs: Any):
        self.nu = nu
        C = kwargs.pop("C", 1.0)
        if C != 1.0:
            self._refuse(f"C={C} (the box is [0, 1])")
        super().__init__(C=1.0, gamma=gamma, eps=eps, max_iter=max_iter, device=device, **kwargs)

    def _check_extra(self) -> None:
        self.nu = _check_nu(self.nu)
        if self.config.C != 1.0:
            self._refuse(f"C={self.config.C} (the box is [0, 1])")

    def _params(self, d: int, nu: Optional[float] = None):
        p = self.config.to_native(d)
        p.one_class_nu = self.nu if nu is None else nu
        return p

    def _rho(self) -> float:
        return self.offset_

    def fit(self, X, y=None, comm=None, resume=None, progress: Optional[Callable] = None, rank_rows=None,
            sample_weight=None) -> "OneClassSVM":
        """Train on the rows of ``X`` (``y`` is ignored).  One rank, from the nu start, unweighted."""
        self._refuse_fit_args(comm, resume, rank_rows, sample_weight)
        self._resolve()
        # kernel="precomputed": X is the (n, n) Gram; decision_function() then takes K(test, train).  A kernel spec:
        # the rows
        X = _train_input(self.config, X)
        n, d = X.shape
        p = self._params(d)
        t0 = time.perf_counter()
        alpha, info, f, setup = self._run(X, np.ones(n, dtype=np.float32), p, progress, want_gradient=True)
        self.wall_time_ = time.perf_counter() - t0
        self.alpha_ = np.ascontiguousarray(np.asarray(alpha, dtype=np.float32).reshape(n))
        self.offset_ = float(info["b"])
        self.train_decision_ = (f.astype(np.float64) - self.offset_).astype(np.float32)
        self._publish_fit(X, self.alpha_, info, p.gamma, setup)
        return self

    def nu_path(self, X, nus: Sequence[float], progress: Optional[Callable] = None) -> dict:
        """One solve per nu on one solver, one ``setup()`` and one resident Gram (``set_nu`` per nu; on the CPU k
        plain solves).  Returns ``{"nu", "rho", "n_support", "outlier_fraction"}`` (the fraction of training rows
        with a negative decision) and keeps ``path_stats_`` (the solves' info dicts: ``gram_reused`` reads
        [False, True, ...]) and ``path_alpha_`` ((k, n)).  The estimator's own fit is left as it is."""
        self._resolve()
        nus = [_check_nu(v) for v in nus]
        if not nus:
            raise ValueError("nu_path needs at least one nu")
        X = _train_input(self.config, X)
        n, d = X.shape
        solves, setup = self._solves(X, np.ones(n, dtype=np.float32), [self._params(d, nu) for nu in nus], progress,
                                     True, between=lambda solver, i: solver.set_nu(nus[i]))
        if self.config.device_kind()[0] == "cuda":
            self.path_setup_info_ = setup
        rho, nsv, out, stats, alphas = [], [], [], [], []
        for alpha, info, f in solves:
            alpha = np.asarray(alpha, dtype=np.float32)
            rho.append(float(info["b"]))
            nsv.append(int(np.count_nonzero(alpha > 0)))
            out.append(float(np.mean(np.asarray(f, dtype=np.float64) - float(info["b"]) < 0)))
            stats.append(info)
            alphas.append(alpha)
        self.path_stats_ = stats
        self.path_alpha_ = np.stack(alphas)
        return {"nu": list(nus), "rho": rho, "n_support": nsv, "outlier_fraction": out}


class LoadedOneClass(_OneClassDecisions, LoadedModel):
    """A one-class model read from the binary text model file."""

    @property
    def offset(self) -> float:
        return self.model.b

    def _rho(self) -> float:
        return self.model.b


def load_one_class(path: str, device: str = "auto") -> LoadedOneClass:
    """The one-class predictor of a model file written by ``OneClassSVM.save``."""
    return LoadedOneClass(load().read_model(path, False), device)
