"""What the estimators and the loaded models share: input conversion, the device string, one predictor holder
and decision path, the per-solve attributes, and the base of the estimators that run one-block working-set
rounds on the resident Gram (SVR, OneClassSVM; the native side of it: csrc/include/dpsvm/problem.hpp).
"""
from __future__ import annotations

import dataclasses
import warnings
from typing import Any

import numpy as np

from .._native import gpu_available, load


def _as_f32_2d(X) -> np.ndarray:
    try:
        import torch

        if isinstance(X, torch.Tensor):
            X = X.detach().to("cpu", dtype=torch.float32).numpy()
    except ImportError:
        pass
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float32))
    if X.ndim != 2:
        raise ValueError(f"X must be 2-D (n_samples, n_features), got shape {X.shape}")
    return X


def _as_1d(y) -> np.ndarray:
    try:
        import torch

        if isinstance(y, torch.Tensor):
            y = y.detach().cpu().numpy()
    except ImportError:
        pass
    return np.asarray(y).reshape(-1)


def _parse_device(dev: str) -> tuple[str, int]:
    """auto | cpu | cuda | cuda:N -> ("cuda", N) or ("cpu", 0); anything else is a ValueError"""
    if dev == "auto":
        return ("cuda", 0) if gpu_available() else ("cpu", 0)
    if dev == "cpu":
        return ("cpu", 0)
    if dev.startswith("cuda"):
        return ("cuda", int(dev.split(":")[1]) if ":" in dev else 0)
    raise ValueError(f"unknown device {dev!r}")


def _pick(table: dict, value: str, name: str) -> int:
    if value not in table:
        raise ValueError(f"{name} must be one of {list(table)}, got {value!r}")
    return table[value]


class _Predicts:
    """The predictor holder of every estimator and loaded model: a device string, the GpuPredictor built on
    first use, one decision path.  A user provides ``_device()`` and ``_native_model()``."""

    _gpu = None
    _multi = False  # k one-vs-rest machines: (n, k) decisions

    def _device(self) -> str:
        return self.config.device

    def _native_model(self):
        return self.to_model()

    def _check_device(self) -> None:
        """an unknown string fails here (construction), not at the first prediction"""
        if self._device() != "auto":
            _parse_device(self._device())

    def _predictor(self):
        """the device predictor, None on the CPU"""
        kind, dev = _parse_device(self._device())
        if kind == "cuda" and self._gpu is None:
            self._gpu = load().GpuPredictor(self._native_model(), dev)
        return self._gpu

    def _decision(self, X) -> np.ndarray:
        """sum_sv coef K(sv, x) - b, float32: (n,), or (n, k) for k machines"""
        X = _as_f32_2d(X)
        d = getattr(self, "n_features_in_", None)
        if d is not None and X.shape[1] != d:
            raise ValueError(f"X has {X.shape[1]} features, model has {d}")
        gp = self._predictor()
        if self._multi:
            out = gp.decision_multi(X) if gp is not None else load().decision_multi_cpu(self._native_model(), X, 0)
        else:
            out = gp.decision(X) if gp is not None else load().decision_cpu(self._native_model(), X, 0)
        return np.asarray(out, dtype=np.float32)


def _publish_solves(est, infos: list, multi: bool = False) -> None:
    """the fitted attributes read off the solves' info dicts: scalars for one machine, stacked for k"""
    if multi:
        est.b_ = np.array([i["b"] for i in infos], dtype=np.float32)
        est.n_iter_ = np.array([i["iters"] for i in infos], dtype=np.int64)
        est.n_rounds_ = np.array([i.get("outer", 0) for i in infos], dtype=np.int64)
        est.stats_ = infos
    else:
        (info,) = infos
        est.b_ = float(info["b"])
        est.n_iter_ = int(info["iters"])
        est.n_rounds_ = int(info.get("outer", 0))
        est.stats_ = info
    est.intercept_ = -est.b_
    est.status_ = int(max(i["status"] for i in infos))
    est.converged_ = bool(all(i["converged"] for i in infos))
    est.fit_time_ = float(sum(i["t_solve"] for i in infos))
    est.setup_time_ = float(infos[0]["t_setup"])


# what the one-block estimators refuse: (the test on the config, what the message names)
_REFUSED = (
    (lambda c: c.clip != "box", "clip={c.clip!r} ({clip_why})"),
    (lambda c: c.solver not in ("auto", "ws"), "solver={c.solver!r} (the pair-at-a-time engines)"),
    (lambda c: c.ws_blocks not in (0, 1), "ws_blocks={c.ws_blocks} (multi-block rounds)"),
    (lambda c: c.shrink_mode() == "on", "shrink='on'"),
    (lambda c: c.ws_recompute == "on", "ws_recompute='on'"),
    (lambda c: c.class_weight is not None, "class_weight (per-row C)"),
    (lambda c: c.force_cache or c.cache_lines or c.host_cache_lines,
     "the kernel-row cache (force_cache / cache_lines / host_cache_lines)"),
    (lambda c: c.engines != "production", "engines='all'"),
    (lambda c: c.x_mode == "partitioned" or c.dp != "auto", "partitioned X / a data-parallel policy"),
    (lambda c: c.exchange == "peer" or c.force_collectives, "the peer exchange / forced collectives"),
    (lambda c: c.checkpoint_path or c.checkpoint_every, "checkpoints"),
)
_RESOLVED = dict(solver="ws", ws_blocks=1, shrink="off", ws_recompute="off")


class _OneBlockEstimator(_Predicts):
    """An estimator whose dual runs on the classifier's one-block working-set rounds over the resident Gram of
    one rank with box clipping, and on nothing else: the settings resolve to ``_RESOLVED``, the rest of
    ``_REFUSED`` raises.  A subclass names itself (``_NAME``, ``_KIND``, ``_RUNS``, ``_CLIP_WHY``), its extra
    hyper-parameter (``_EXTRA``), checks it (``_check_extra``) and sets it in the native params (``_params``)."""

    _NAME = _KIND = _RUNS = _CLIP_WHY = _EXTRA = ""

    def __init__(self, **config: Any):
        from .svc import SVCConfig

        config.setdefault("clip", "box")
        self.config = SVCConfig(**config)
        self._resolve()
        self._model = None

    @classmethod
    def _refuse(cls, what: str) -> None:
        raise NotImplementedError(f"{cls._NAME}: {what} is not implemented for {cls._KIND} ({cls._RUNS})")

    def _check_extra(self) -> None:
        pass

    def _resolve(self) -> None:
        """refuse what the estimator does not run, resolve the rest (before any native or device state exists)"""
        cfg = self.config
        self._check_extra()
        _parse_device(cfg.device)
        for refused, what in _REFUSED:
            if refused(cfg):
                self._refuse(what.format(c=cfg, clip_why=self._CLIP_WHY))
        for name, value in _RESOLVED.items():
            setattr(cfg, name, value)

    def _refuse_fit_args(self, comm, resume, rank_rows, sample_weight) -> None:
        """one rank, from the estimator's own start, unweighted"""
        for name, val in (("comm", comm), ("resume", resume), ("rank_rows", rank_rows),
                          ("sample_weight", sample_weight)):
            if val is not None:
                self._refuse(name)

    def _run(self, X: np.ndarray, y_native: np.ndarray, p, progress, want_gradient: bool):
        """one solve on the configured device -> alpha, info, the gradient (or None), the setup info"""
        C = load()
        kind, dev = self.config.device_kind()
        f = None
        if kind == "cuda":
            solver = C.GpuSolver(p, None, dev)  # dropped after the solve, with its resident Gram
            setup = solver.setup(X, len(X), y_native)
            alpha, info = solver.solve(None, progress)
            if want_gradient:
                f = solver.gradient()
            del solver
            info = dict(info)
        else:
            setup = {"iteration": "cpu", "engine_note": C.problem_note(p)}
            alpha, info = C.solve_cpu(X, y_native, p, None, None, progress, None)
            info = dict(info)
            if want_gradient:
                f = info.pop("f")
        self.device_ = f"{kind}:{dev}" if kind == "cuda" else "cpu"
        return alpha, info, None if f is None else np.asarray(f, dtype=np.float32), setup

    def _publish_fit(self, X: np.ndarray, coef: np.ndarray, info: dict, gamma: float, setup: dict) -> None:
        """the attributes of a fit whose model is sum_i coef_i K(x_i, x) - b; called by fit()"""
        self.setup_info_ = setup
        _publish_solves(self, [info])
        self.gamma_ = gamma
        self.n_features_in_ = X.shape[1]
        self.support_ = np.nonzero(coef != 0)[0]
        self.support_vectors_ = X[self.support_]
        self.dual_coef_ = coef[self.support_].astype(np.float32)
        self.n_support_ = int(len(self.support_))
        self._X_train, self._coef = X, coef
        self._model = None
        self._gpu = None
        if self.status_ == 2:
            warnings.warn(f"stopped at max_iter with gap {info['b_lo'] - info['b_hi']:.3g} > 2 eps: raise max_iter "
                          "to converge", RuntimeWarning, stacklevel=3)

    def to_model(self):
        """the binary model of coef: alpha = |coef|, y = sign(coef) (rows with coef = 0 are no SVs)"""
        if self._model is None:
            coef = getattr(self, "_coef", None)
            if coef is None:
                raise RuntimeError(f"to_model() needs a fitted {self._NAME}")
            y = np.where(coef < 0, -1.0, 1.0).astype(np.float32)
            self._model = load().make_model(self._X_train, y, np.abs(coef).astype(np.float32), self.b_, self.gamma_)
        return self._model

    def save(self, path: str, precision: int = 9) -> None:
        """Write the binary text model (gamma, b, then |coef|, sign(coef), x per SV)."""
        load().write_model(path, self.to_model(), precision, False)

    def get_params(self, deep: bool = True) -> dict:
        out = dataclasses.asdict(self.config)
        out[self._EXTRA] = getattr(self, self._EXTRA)
        return out
