"""SVC: the estimator-level API over the native MI355X solver.

Reference capability map (farshid83/dpsvm):
  fit()                -> svmTrainMain.cpp:142-365 (GPU/MPI trainer) or seq.cpp (CPU)
  decision_function()  -> svmTrain.cu:633-665 (training accuracy) / seq_test.cpp:187-210
  save() / load_model()-> svmTrainMain.cpp:386-416 model writer, seq_test.cpp:212-249 reader
Labels: the reference requires +1/-1 (svmTrain.cu:58,73); any two distinct
labels are accepted here and mapped (classes_[1] -> +1), like scikit-learn.
More than two labels train one-vs-rest machines (no reference counterpart):
one device solver, one resident Gram, a label swap per machine, and one
multi-output decision GEMM over the union of the machines' support vectors.
"""
from __future__ import annotations

import dataclasses
import math
import time
from dataclasses import dataclass
from typing import Any, Callable, Optional

import numpy as np

from .._native import load, load_quarantine
from ._base import (_Kernel, _Predicts, _as_1d, _config_params, _kernel_code, _parse_device, _pick, _publish_solves,
                    _refuse_precomputed, _stamp_kernel, _train_input)


_CLIP = {"independent": 0, "box": 1}
_DP = {"auto": 0, "shard": 1, "replicate": 2}           # SolverParams.dp_policy
_GRAM = {"auto": 0, "f32": 1, "split": 2}               # SolverParams.gram_precision
_AUTO_ON_OFF = {"auto": 0, "on": 1, "off": 2}
# SVCConfig fields whose SolverParams attribute has the same name: the enums by their table ...
_ENUMS = {
    "x_mode": {"auto": 0, "replicated": 1, "partitioned": 2},
    "exchange": {"auto": 0, "allreduce": 1, "peer": 2},
    "persist": {"auto": 0, "off": 1, "on": 2},
    "cache_engine": {"fused": 0, "chain": 1},
    "engines": {"production": 0, "all": 1},
    "xch_mem": {"auto": 0, "uncached": 1, "coarse": 2},
    "solver": {"auto": 0, "smo": 1, "ws": 2},
    "ws_recompute": _AUTO_ON_OFF,
    "eta": {"x": 0, "gram": 1},
    "gram_adapt": _AUTO_ON_OFF,
}
# ... and the plain ones by their type
_PLAIN = {
    float: ("C", "eps", "tau", "cache_mb", "cache_frac", "xch_timeout_s", "watchdog_s", "ws_rel", "ws_t_halve",
            "gram_cold_tau"),
    int: ("max_iter", "cache_lines", "host_cache_lines", "spec_rows", "graph_block", "log_every", "checkpoint_every",
          "persist_block", "cache_groups", "rows_per_group", "xch_poll_batch", "xch_sleep", "xch_stride",
          "census_groups", "ws_size", "ws_new", "ws_blocks", "ws_inner", "ws_wss", "ws_block"),
    bool: ("use_graph", "verbose", "force_collectives", "force_cache", "verify_ranks"),
}


def _gradient(solver, info: dict) -> np.ndarray:
    """the gradient f after a solve: the live GpuSolver's, or (solver None) the CPU solve's info["f"]"""
    return np.asarray(solver.gradient() if solver is not None else info["f"], dtype=np.float32)


def _write_platt(path: str, A, B) -> None:
    """the sidecar ``path + ".platt"`` of a model file: "dpsvm-platt <k>", the k A values, the k B values
    (comma-separated, 17 significant digits); without sigmoids a stale one is removed"""
    import os

    side = path + ".platt"
    if A is None:
        if os.path.exists(side):
            os.remove(side)
        return
    A, B = np.atleast_1d(A), np.atleast_1d(B)
    with open(side, "w") as f:
        f.write(f"dpsvm-platt {len(A)}\n")
        for v in (A, B):
            f.write(",".join("%.17g" % float(x) for x in v) + "\n")


def _read_platt(path: str, k: int):
    """(A, B) float64 (k,) of the sidecar of the model file ``path``, None when there is none"""
    import os

    side = path + ".platt"
    if not os.path.exists(side):
        return None
    with open(side) as f:
        lines = f.read().split("\n")
    head = lines[0].split()
    if len(lines) < 3 or len(head) != 2 or head[0] != "dpsvm-platt" or int(head[1]) != k:
        raise ValueError(f"{side}: not the Platt sidecar of a model of {k} machine(s)")
    A, B = (np.array([float(v) for v in ln.split(",")], dtype=np.float64) for ln in lines[1:3])
    if len(A) != k or len(B) != k:
        raise ValueError(f"{side}: needs {k} A and {k} B values")
    return A, B


@dataclass
class SVCConfig:
    """Solver configuration (mirrors the svmTrain flags)."""

    C: float = 1.0                  # -c (reference default 1)
    gamma: Optional[float] = None   # -g; None -> 1/d (reference: integer 1/d, Q1)
    eps: float = 1e-3               # -e
    max_iter: int = 150000          # -n
    clip: str = "independent"       # reference clipping; "box" = LIBSVM joint box
    tau: float = 1e-12              # eta floor (Q4)
    cache_lines: int = 0            # -s (0 = auto: fill HBM; dense Gram when it fits)
    cache_mb: float = 0.0
    cache_frac: float = 0.80
    host_cache_lines: int = 0       # pinned host tier lines (LRU mode; 0 = off)
    spec_rows: int = 14             # speculative rows per X pass (LRU mode)
    graph_block: int = 64           # SMO iterations per hipGraph
    use_graph: bool = True
    x_mode: str = "auto"            # auto | replicated | partitioned
    log_every: int = 0
    checkpoint_path: Optional[str] = None
    checkpoint_every: int = 0
    device: str = "auto"            # auto | cpu | cuda | cuda:N
    verbose: bool = False
    force_collectives: bool = False  # run the per-iteration collective even with one rank (tests)
    exchange: str = "auto"          # per-iteration key exchange (dense mode): auto | allreduce | peer
    persist: str = "auto"           # engine: auto | off (one launch per iteration) | on (persistent, dense or cache mode)
    persist_block: int = 2048       # SMO iterations per persistent launch
    # engine / geometry selection (all recorded in setup_info_ and the run summaries)
    dp: str = "auto"                # world > 1: auto | shard (rows split) | replicate (every rank solves it all)
    force_cache: bool = False       # kernel-row cache mode even when the Gram fits
    cache_engine: str = "fused"     # cache mode, one launch per iteration: fused | chain
    # production (ws-dense, ws-cache, persistent-dense, fused-dense) | all: also the quarantined
    # pair-at-a-time engines for a non-resident Gram / partitioned X (persistent-cache, fused-cache, chain;
    # host_cache_lines and cache_engine=chain need it) — tests and A/B probes (device_state.hpp kQuarantineTable)
    engines: str = "production"
    cache_groups: int = 256         # cache mode workgroups per rank
    rows_per_group: int = 0         # rows per workgroup of the fused/persistent engines (0 auto; multiple of 256)
    xch_poll_batch: int = 0         # peer exchange: publications per lane per poll round (0 auto)
    xch_sleep: int = 1
    xch_stride: int = 4
    xch_mem: str = "auto"           # auto | uncached | coarse
    xch_timeout_s: float = 120.0    # give-up bound of one in-kernel poll (then the solve fails)
    watchdog_s: float = 0.0  # 0: auto (1800 s; adaptive to the block time at world > 1)
    census_groups: int = 0          # residency census grid (tests)
    verify_ranks: bool = True       # cross-rank alpha digest after each solve (world > 1)
    # solver: auto (ws from 50k rows, else smo) | smo (pair-at-a-time engines, the reference's trajectory) |
    # ws (working-set rounds: the reference's pair rule on a q-row sub-problem
    # in LDS, the same global stop test; ws_*.hip)
    solver: str = "auto"
    ws_size: int = 192              # working-set rows (<= 192)
    ws_new: int = 0                 # rows replaced per one-block round (0: auto, ws_size from 128 padded features, else 3/4)
    ws_rel: float = 0.3             # sub-problem tolerance relative to the global gap (< 1)
    # working-set engines: up to P sub-problems per round (1..128, P x ws_size <= 6144).  0 auto, from 50k rows:
    # uncoupled (numerically diagonal) ws-dense kernels 128 blocks of 48 rows (6144-row union; 64 x 48 = 3072
    # when ranks sharing one device would not leave room for the peer exchange's producers), coupled kernels
    # and ws-cache 32 blocks of 96 (3072-row union); below 50k rows 1.  Adaptive —
    # halved after every damped round (coupled blocks), then the one-block round kernels (ws_*.hip;
    # kWsMaxBlocks / kWsMaxAll in include/dpsvm/device_state.hpp)
    ws_blocks: int = 0
    ws_inner: int = 0               # pair steps per round at most (0: 4 * ws_size)
    ws_wss: int = 0                 # sub-problem pair choice: 0 auto (second order on coupled kernels), 1 first, 2 second
    ws_block: int = 8               # rounds per hipGraph block (or per persistent-round launch)
    # ws-cache rounds without the kernel-row cache (ws_recompute.hip: the round's kernel rows recomputed inside
    # the f update, the sub-Gram straight from X): auto (one GPU, one block, d <= 64) | on | off
    ws_recompute: str = "auto"
    # one GPU: LIBSVM-style shrinking as problem reduction (solve_shrinking: phases on the rows that can
    # still violate, the rest of the gradient updated by one predict GEMM per phase).  auto: on where it
    # pays — one GPU, working-set rounds, the whole Gram not resident (C.shrink_auto) | on | off
    shrink: str = "auto"
    ws_t_halve: float = 0.9         # multi-block: a round damped below this t halves the block count
    ws_clip_fallback: bool = True   # multi-block, independent clipping: one block per round after a clip
    eta: str = "x"                  # pair engines' K(hi, lo): x (from the X rows) | gram (resident Gram)
    # Gram / kernel-row GEMM arithmetic: auto (split for the working-set engines, f32 for the pair engines),
    # f32 (f32-input MFMA), split (fp16 MFMA over hi/lo split operands: fp32 accuracy, 3/16 of the MFMA time)
    gram: str = "auto"
    # adaptive resident split Gram (ws-dense, docs/DESIGN.md §13): one-product tiles where every element is
    # provably within gram_cold_tau of the three-product value, the rest recomputed — auto (on when a row
    # sample passes the bound) | on | off
    gram_adapt: str = "auto"
    gram_cold_tau: float = 2.0 ** -22
    # per-row C (C_i = C * w_i): None | "balanced" (n / (2 n_c) per class, scikit-learn's formula; one-vs-rest:
    # each machine's two sides) | {label: weight} (missing labels 1).  Multiplied by fit(sample_weight=).  Any
    # weights run the working-set engines on one rank (solver auto -> ws, shrink / ws_recompute auto -> off)
    class_weight: Any = None
    # "rbf" (gamma; fit takes X) | "precomputed" (LIBSVM -t 4): fit takes the (n, n) Gram of any kernel and never X,
    # decision_function K(test, train); gamma is ignored.  One-block working-set rounds on the resident Gram of one
    # rank with box clipping (general-diagonal sub-problem kernels, docs/DESIGN.md §20); settings resolve as for a
    # weighted fit plus ws_blocks=1, the rest is refused (README "Precomputed kernels").  Init-only: it is no
    # solver knob but what fit() and decision_function() take, so it stays off dataclasses.fields(), the list of
    # settings that map one to one onto SolverParams (get_params() reports it when it is not "rbf").
    # Or a kernel spec — Linear(), Poly(degree, coef0), Sigmoid(coef0) — in place of a string: fit takes X, the
    # Gram of (gamma x.y + coef0)^degree etc. is built on the device straight into the solver's lines and solved
    # as a precomputed one (same resolutions and refusals); the model keeps its rows and predicts from X
    # (docs/DESIGN.md §21).  gamma stays this config's field (default 1 / d)
    kernel: dataclasses.InitVar[Any] = "rbf"

    def __post_init__(self, kernel: Any = "rbf"):
        _kernel_code(kernel)
        self.kernel = kernel

    def shrink_mode(self) -> str:
        s = self.shrink
        if s is True or s is False:
            return "on" if s else "off"
        if s not in ("auto", "on", "off"):
            raise ValueError(f"shrink must be auto, on or off (got {s!r})")
        return s

    def resolved_gamma(self, d: int) -> float:
        return float(self.gamma) if self.gamma is not None and self.gamma >= 0 else 1.0 / float(d)

    def to_native(self, d: int):
        C = load()
        if not self.C > 0:
            raise ValueError("C must be > 0")
        if self.rows_per_group % 256:
            raise ValueError("rows_per_group must be a multiple of 256")
        p = C.SolverParams()
        for cast, names in _PLAIN.items():
            for name in names:
                setattr(p, name, cast(getattr(self, name)))
        for name, table in _ENUMS.items():
            setattr(p, name, _pick(table, getattr(self, name), name))
        p.gamma = self.resolved_gamma(d)
        p.clip = C.ClipMode.box if _pick(_CLIP, self.clip, "clip") else C.ClipMode.independent
        p.checkpoint_path = self.checkpoint_path or ""
        p.dp_policy = _pick(_DP, self.dp, "dp")
        p.gram_precision = _pick(_GRAM, self.gram, "gram")
        p.ws_clip_fallback = int(bool(self.ws_clip_fallback))
        p.kernel = _kernel_code(self.kernel)
        if p.kernel:
            _refuse_precomputed(self)
            p.solver, p.ws_recompute, p.ws_blocks = 2, 2, 1
        return p

    def weighted_params(self, p, comm=None, resume=None, rank_rows=None) -> str:
        """Resolve / refuse the settings of a solve with per-row C; returns the note for ``engine_note``."""
        for name, val in (("comm", comm), ("resume", resume), ("rank_rows", rank_rows),
                          ("checkpoint_path", self.checkpoint_path)):
            if val:
                raise NotImplementedError(f"sample / class weights (per-row C) run on one rank from a cold start "
                                          f"without checkpoints: {name} is not supported")
        if self.solver == "smo":
            raise NotImplementedError("sample / class weights need the working-set engines: the pair-at-a-time "
                                      "engines (solver='smo') keep bit parity with the reference and take one C")
        if self.shrink_mode() == "on":
            raise NotImplementedError("sample / class weights: shrink='on' is not supported (the shrinking phases "
                                      "subset the rows, not the weights)")
        if self.ws_recompute == "on":
            raise NotImplementedError("sample / class weights: ws_recompute='on' is not supported (its selection "
                                      "takes one C)")
        note = "per-row C"
        if self.solver == "auto":
            note += ": solver auto -> ws"
        p.solver = 2
        p.ws_recompute = 2
        return note

    def device_kind(self) -> tuple[str, int]:
        return _parse_device(self.device)


class SVC(_Predicts):
    """RBF C-SVM trained by modified SMO on MI355X (or the CPU).

    Attributes after fit: ``alpha_`` (dual variables, len n), ``b_`` (threshold:
    decision = sum alpha_i y_i K(x_i, x) - b), ``intercept_`` (= -b_),
    ``support_`` (indices with alpha > 0), ``support_vectors_``, ``dual_coef_``
    (alpha*y of the SVs), ``n_iter_``, ``status_``, ``fit_time_`` (SMO loop
    seconds, the reference's timed region), ``stats_`` (cache / pass counters).

    More than two distinct labels: k one-vs-rest machines (machine c separates
    ``classes_[c]`` from the rest).  Then ``alpha_`` is (k, n), ``b_`` /
    ``intercept_`` / ``n_iter_`` (k,), ``support_`` / ``support_vectors_`` the
    union of the machines' SVs, ``dual_coef_`` (k, nsv), ``stats_`` a list of
    the k solves' dicts, ``fit_time_`` their sum, ``status_`` their maximum;
    ``decision_function`` returns (n, k) and ``predict`` the class of the
    largest value (ties: the lowest class index).

    Sample / class weights (``fit(sample_weight=)``, ``class_weight``): row i's
    box is ``0 <= alpha_i <= C * w_i``; ``row_C_`` holds the bounds ((n,), or
    (k, n)), ``n_bounded_`` counts ``alpha_i == C_i > 0``.  ``cross_val_decision``
    / ``cross_val_score``: k folds as k solves on one resident Gram.

    Probabilities (``fit(probability=cv)``, docs/DESIGN.md §16): per machine the
    full-data solve and ``cv`` fold solves on that Gram; ``cv_decision_`` holds the
    out-of-fold decisions ((n,), or (n, k)), ``probA_`` / ``probB_`` the Platt
    sigmoids fitted on them (float64; (k,) for k machines), ``platt_stats_`` the
    fits' ``iters`` / ``evals`` / ``fval`` / ``status``, ``cv_stats_`` the fold
    solves' dicts (per machine); ``stats_`` stays the full-data solves.
    ``predict_proba`` needs them; ``save`` writes them to ``path + ".platt"``.
    """

    def __init__(self, C: float = 1.0, gamma: Optional[float] = None, eps: float = 1e-3,
                 max_iter: int = 150000, device: str = "auto", **kwargs: Any):
        on_gram = _Kernel(kwargs.get("kernel", "rbf")).on_gram
        if on_gram:
            kwargs.setdefault("clip", "box")
        self.config = SVCConfig(C=C, gamma=gamma, eps=eps, max_iter=max_iter, device=device, **kwargs)
        if on_gram:
            _refuse_precomputed(self.config)
        self._model = None
        self._multi = False
        self.classes_ = np.array([-1.0, 1.0], dtype=np.float32)

    # ------------------------------------------------------------------ labels
    def _encode(self, y) -> np.ndarray:
        y = _as_1d(y)
        u = np.unique(y)
        if len(u) > 2:
            raise ValueError(f"binary classifier: got {len(u)} classes")
        if len(u) == 2 and set(u.tolist()) <= {-1, 1}:
            self.classes_ = np.array([-1.0, 1.0], dtype=np.float32)
            return np.where(y > 0, 1.0, -1.0).astype(np.float32)
        if len(u) == 1:
            self.classes_ = np.array([u[0], u[0]])
            return np.ones(len(y), dtype=np.float32) * (1.0 if (u[0] > 0 if np.isreal(u[0]) else True) else -1.0)
        self.classes_ = u
        return np.where(y == u[1], 1.0, -1.0).astype(np.float32)

    def _decode(self, s: np.ndarray) -> np.ndarray:
        if np.array_equal(self.classes_, np.array([-1.0, 1.0], dtype=np.float32)):
            return s.astype(np.float32)
        return np.where(s > 0, self.classes_[-1], self.classes_[0])

    def _use_shrink(self, p, n: int, d: int, dev: int, comm=None) -> bool:
        """collective at world > 1 (every rank calls; agreed)"""
        mode = self.config.shrink_mode()
        return mode == "on" or (mode == "auto" and bool(load().shrink_auto(p, n, d, dev, comm)))

    # ------------------------------------------------------------------ weights
    @staticmethod
    def _sample_weight(sample_weight, n: int) -> np.ndarray:
        """float64 (n,), validated: finite and >= 0 (ones when None)"""
        if sample_weight is None:
            return np.ones(n, dtype=np.float64)
        w = np.asarray(_as_1d(sample_weight), dtype=np.float64)
        if w.shape[0] != n:
            raise ValueError(f"sample_weight has {w.shape[0]} entries, X has {n} rows")
        if not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError("sample_weight must be finite and >= 0")
        return w

    @staticmethod
    def _class_dict(cw, y: np.ndarray) -> np.ndarray:
        """a {label: weight} dict as per-row weights (missing labels 1)"""
        out = np.ones(len(y), dtype=np.float64)
        for lab, wv in cw.items():
            wv = float(wv)
            if not math.isfinite(wv) or wv < 0:
                raise ValueError("class_weight values must be finite and >= 0")
            out[y == lab] = wv
        return out

    def _row_C(self, w64: np.ndarray, ys: np.ndarray) -> np.ndarray:
        """C_i = C * w_i in float32; each side of ys needs a positive bound"""
        rc = (np.float32(self.config.C) * w64.astype(np.float32)).astype(np.float32)
        if not np.all(np.isfinite(rc)):
            raise ValueError("C * weight overflows float32")
        if not (np.any(rc[ys > 0] > 0) and np.any(rc[ys <= 0] > 0)):
            raise ValueError("weights leave one class without a row of positive C_i")
        return rc

    def _weights(self, y: np.ndarray, Ys: np.ndarray, sample_weight) -> Optional[np.ndarray]:
        """(k, n) float64 row weights of the machines Ys (class weight x sample weight), None without any.
        ``balanced``: each machine's two sides; a dict: a row's own label y, in every machine."""
        cw = self.config.class_weight
        if cw is None and sample_weight is None:
            return None
        k, n = Ys.shape
        W = np.tile(self._sample_weight(sample_weight, n), (k, 1))
        if cw is None:
            return W
        if isinstance(cw, dict):
            return W * self._class_dict(cw, y)[None, :]
        if not isinstance(cw, str) or cw != "balanced":
            raise ValueError(f"class_weight must be None, 'balanced' or a dict (got {cw!r})")
        for c in range(k):
            n_pos = int(np.sum(Ys[c] > 0))
            if n_pos == 0 or n_pos == n:
                raise ValueError("class_weight='balanced' needs both classes")
            W[c] *= np.where(Ys[c] > 0, n / (2.0 * n_pos), n / (2.0 * (n - n_pos)))
        return W

    def _problem(self, d: int, y: np.ndarray, Ys: np.ndarray, sample_weight, comm=None, resume=None, rank_rows=None):
        """the native params, the machines' row bounds (k, n) or None, and a weighted solve's engine note"""
        p = self.config.to_native(d)
        W = self._weights(y, Ys, sample_weight)
        if W is None:
            return p, None, None
        RC = np.stack([self._row_C(W[c], Ys[c]) for c in range(len(Ys))])  # any weights: no shortcut for all ones
        return p, RC, self.config.weighted_params(p, comm, resume, rank_rows)

    # ------------------------------------------------------------------ fit
    def _solve_machines(self, X, Ys: np.ndarray, RC, p, note=None, comm=None,
                        resume=None, progress=None, rank_rows=None, hook=None, keep=False, lab=None):
        """The solves of one fit on one training input X (_train_input): machine c has the labels ``Ys[c]`` and the
        row bounds ``RC[c]`` (RC None: the scalar C; an entry None: the scalar C for that solve); ``Ys`` (1, n)
        under more rows of RC is one set of labels for all of them (the folds of a cross-validation); ``lab[c]``:
        the row of Ys that solve c uses (the full-data solve and the folds of each machine of a probability fit).
        On the GPU one solver: the input's setup (upload, norms, operand prep, engine choice) once, then per
        machine set_labels (after the first), set_row_C (with RC) and solve; the resident Gram built by the first
        solve is kept by the swaps after it.  ``hook(c, solver, info)`` runs after solve c on the live GpuSolver
        (on the CPU: solver None, info["f"] the gradient).  Returns the alphas, the info dicts, the setup info (on
        the CPU the input's, None for RBF rows) and, with ``keep``, the GpuSolver (else it is dropped here, with
        its Gram)."""
        C = load()
        k, n = Ys.shape
        m = k if RC is None else len(RC)
        if lab is None:
            lab = list(range(m)) if k > 1 else [0] * m
        ck = C.read_checkpoint(resume) if isinstance(resume, str) else resume
        kind, dev = self.config.device_kind()
        alphas, infos, setup, solver = [], [], None, None
        if (kind == "cuda" and rank_rows is None and RC is None and X.may_shrink
                and self._use_shrink(p, n, X.shape[1], dev, comm)):
            for c in range(m):  # ShrinkingSolver has no label swap: one per machine
                shr = C.ShrinkingSolver(p, comm, dev)
                s = shr.setup(X.kept_rows(), Ys[c])  # the whole-problem phases' solver; iteration "ws+shrinking"
                a, info = shr.solve(ck, progress)
                if c == 0:
                    setup = s
                    if m == 1:
                        setup["engine_note"] = f"{info['shrink_phases']} shrinking phases: {info['phase_log']}"
                alphas.append(a)
                infos.append(dict(info))
                del shr
        elif kind == "cuda":
            solver = C.GpuSolver(p, comm, dev)
            setup = X.setup(solver, Ys[0])
            if note:
                en = setup.get("engine_note", "")
                setup["engine_note"] = (en + "; " if en else "") + note
            for c in range(m):
                if c and lab[c] != lab[c - 1]:
                    solver.set_labels(Ys[lab[c]])
                if RC is not None:
                    solver.set_row_C(RC[c])
                a, info = solver.solve(ck, progress)
                if hook is not None:
                    hook(c, solver, info)
                alphas.append(a)
                infos.append(dict(info))
        else:
            if rank_rows is not None:
                raise ValueError("partitioned X needs the GPU solver")
            setup = X.cpu_setup(p)
            for c in range(m):
                a, info = X.solve_cpu(p, Ys[lab[c]], None if RC is None else RC[c], comm, ck, progress)
                info = dict(info)
                if hook is not None:
                    hook(c, None, info)
                info.pop("f", None)
                alphas.append(a)
                infos.append(info)
        return alphas, infos, setup, solver if keep else None

    def _cv_solves(self, X, Ys: np.ndarray, W: Optional[np.ndarray], p, cv: int, seed: int,
                   full: Optional[list] = None, note=None, progress=None, keep=False, want_grads=False):
        """Per machine c (labels ``Ys[c]``, weights ``W[c]`` or ones): with ``full`` the full-data solve under the
        bounds ``full[c]`` (None: the scalar C), then the ``cv`` fold solves, each with the fold's weights zeroed
        (C_i = 0: alpha_i stays 0, the row is out of the problem) — all through _solve_machines, so on the GPU on
        one solver, one setup() and one resident Gram.  There a held-out row's decision value is f_i + y_i - b,
        its gradient entry as every round's f update kept it: written on the device into the solver's slot c
        (holdout_decision_kernel), downloaded once per machine, and with ``full`` fitted there by
        platt_fit_kernel against the machine's labels.  On the CPU the decisions come from the input's holdout_cpu
        and the fit from platt_fit_cpu.  Folds: ``cv_folds(n, cv, seed)``, the same for every machine.  Returns the
        out-of-fold decisions (k, n), the folds, the Platt fits (k dicts; None without ``full``), the full-data
        solves' alphas and dicts, the folds' dicts per machine, the setup info, the kept GpuSolver and, with
        ``want_grads``, the full-data solves' gradients (k arrays; else None)."""
        C = load()
        k, n = Ys.shape
        folds = self.cv_folds(n, cv, seed)
        RC, lab, role = [], [], []  # solve i: machine role[i][0], fold role[i][1] (-1: the full-data solve)
        for c in range(k):
            if full is not None:
                RC.append(full[c])
                lab.append(c)
                role.append((c, -1))
            w = np.ones(n, dtype=np.float64) if W is None else W[c]
            for j, fold in enumerate(folds):
                wf = w.copy()
                wf[fold] = 0.0
                RC.append(self._row_C(wf, Ys[c]))
                lab.append(c)
                role.append((c, j))
        rows = [np.ascontiguousarray(fold, dtype=np.int32) for fold in folds]
        dec = np.zeros((k, n), dtype=np.float32)
        platt = [None] * k
        on_device = []
        grads = [None] * k if want_grads else None

        def hook(i, solver, info):  # cold solves (alpha = 0, f = -y): the gradient is the whole decision
            c, j = role[i]
            if j < 0 and want_grads:
                grads[c] = _gradient(solver, info)
            if solver is None:  # (the CPU solver: only the gradients)
                return
            if j >= 0:
                solver.holdout_decisions(rows[j], float(info["b"]), c)
            if i + 1 == len(role) or role[i + 1][0] != c:  # machine c's last solve: its labels are still current
                if full is not None:
                    platt[c] = dict(solver.platt_fit(c))
                dec[c] = solver.holdout(c)
                on_device.append(c)

        alphas, infos, setup, solver = self._solve_machines(X, Ys, RC, p, note, progress=progress, hook=hook,
                                                            keep=keep, lab=lab)
        if not on_device:
            for i, (c, j) in enumerate(role):
                if j >= 0:
                    dec[c, folds[j]] = X.holdout_cpu(p, Ys[c], alphas[i], infos[i]["b"], folds[j])
            if full is not None:
                platt = [dict(C.platt_fit_cpu(dec[c], Ys[c])) for c in range(k)]
        is_full = [j < 0 for _, j in role]
        f_alphas = [a for a, f in zip(alphas, is_full) if f]
        f_infos = [s for s, f in zip(infos, is_full) if f]
        cv_infos = [[s for s, (cc, j) in zip(infos, role) if cc == c and j >= 0] for c in range(k)]
        return dec, folds, (platt if full is not None else None), f_alphas, f_infos, cv_infos, setup, solver, grads

    def _fit_solves(self, X, y, Ys, sample_weight, probability: int, seed: int, comm, resume, progress, rank_rows,
                    keep: bool, want_grads: bool):
        """The solves of fit(): the machines of Ys, or with ``probability`` folds each machine's full-data solve
        and fold solves on one Gram (_cv_solves) with the Platt fits.  Returns the native params, the machines'
        row bounds, the alphas, the full-data solves' dicts, the setup info, the kept GpuSolver, the
        probability results (None without) and, with ``want_grads``, the full-data solves' gradients (else None)."""
        p, RC, note = self._problem(X.shape[1], y, Ys, sample_weight, comm, resume, rank_rows)
        if not probability:
            grads = hook = None
            if want_grads:
                grads = [None] * len(Ys)

                def hook(c, solver, info):  # machine c's gradient after its solve
                    grads[c] = _gradient(solver, info)
            alphas, infos, setup, solver = self._solve_machines(X, Ys, RC, p, note, comm, resume, progress,
                                                                rank_rows, hook=hook, keep=keep)
            return p, RC, alphas, infos, setup, solver, None, grads
        if RC is None:  # resolved as a weighted fit; the full-data solves keep the scalar C
            note = self.config.weighted_params(p, comm, resume, rank_rows)
        full = [None] * len(Ys) if RC is None else list(RC)
        W = self._weights(y, Ys, sample_weight)
        dec, folds, platt, alphas, infos, cv_infos, setup, solver, grads = self._cv_solves(
            X, Ys, W, p, probability, seed, full, note, progress, keep, want_grads)
        return p, RC, alphas, infos, setup, solver, (dec, folds, platt, cv_infos), grads

    def _publish_proba(self, proba) -> None:
        """cv_decision_, cv_stats_, cv_folds_, probA_, probB_, platt_stats_ of a probability fit (else cleared)"""
        if proba is None:
            self.probA_ = self.probB_ = self.platt_stats_ = self.cv_decision_ = None
            return
        dec, folds, platt, cv_infos = proba
        multi = self._multi
        self.cv_decision_ = np.ascontiguousarray(dec.T) if multi else dec[0]
        self.cv_stats_ = cv_infos if multi else cv_infos[0]
        self.cv_folds_ = folds
        A = np.array([f["A"] for f in platt], dtype=np.float64)
        B = np.array([f["B"] for f in platt], dtype=np.float64)
        self.probA_, self.probB_ = (A, B) if multi else (np.float64(A[0]), np.float64(B[0]))
        stats = [{key: f[key] for key in ("iters", "evals", "fval", "status")} for f in platt]
        self.platt_stats_ = stats if multi else stats[0]
        bad = [(c, f["status"]) for c, f in enumerate(platt) if f["status"] != 0]
        if bad:
            import warnings

            why = {1: "its line search failed", 2: "it stopped at 100 Newton steps"}
            warnings.warn("the Platt sigmoid fit did not converge: " +
                          "; ".join(f"machine {c}: {why.get(s, s)}" for c, s in bad), RuntimeWarning, stacklevel=3)

    def fit(self, X, y, comm=None, resume=None, progress: Optional[Callable] = None,
            rank_rows: Optional[int] = None, sample_weight=None, probability: int = 0,
            probability_seed: int = 0) -> "SVC":
        """Train.  ``comm``: a native communicator (see dpsvm_amd.parallel) for
        multi-rank training; ``resume``: checkpoint path or native Checkpoint;
        ``sample_weight``: per-row multipliers of C (with ``class_weight``);
        ``probability``: folds of the cross-validation whose out-of-fold
        decisions fit each machine's Platt sigmoid for ``predict_proba`` (0: off;
        LIBSVM uses 5; folds ``cv_folds(n, probability, probability_seed)``).
        The settings then resolve as for a weighted fit, and the full-data solve
        and the folds of every machine run on one resident Gram.

        More than two labels: one-vs-rest, k machines on one input, the GpuSolver
        dropped (with its resident Gram) after the last.  kernel="precomputed":
        X is the (n, n) Gram K of any kernel (symmetric; a GPU torch tensor is
        passed by pointer, anything else uploaded); there are no rows to keep:
        ``support_``, ``dual_coef_``, ``alpha_``, ``b_`` / ``intercept_`` and
        ``probA_`` / ``probB_`` are the model, ``gamma_`` is None, and prediction
        takes K(test, train).  A kernel spec (Linear / Poly / Sigmoid): X is the
        rows; the solver builds the Gram from them into its lines, everything else
        as for a precomputed kernel, and the model keeps its rows
        (``support_vectors_``, ``save``; prediction takes test rows).  Every case
        runs on one GpuSolver and one setup: k solves with ``set_labels`` /
        ``set_row_C``.  Only two classes under the RBF kernel — the reference's
        trainer — take ``comm``, ``resume`` and ``rank_rows``, keep the solver
        (``train_accuracy`` on the device) and print ``log_every``'s lines."""
        probability = int(probability)
        if probability != 0 and probability < 2:
            raise ValueError(f"probability is the number of folds: 0 (off) or >= 2, got {probability}")
        cfg = self.config
        kern = self._kernel()
        rank_args = dict(comm=comm, resume=resume, rank_rows=rank_rows)
        if kern.on_gram:
            _refuse_precomputed(cfg, **rank_args)
        elif cfg.engines == "all" or cfg.host_cache_lines or cfg.cache_engine == "chain":
            load_quarantine()  # the quarantined pair-at-a-time cache engines (plugin)
        inp = _train_input(cfg, X)
        y1 = _as_1d(y)
        classes = np.unique(y1)
        multi = len(classes) > 2
        case = "gram" if kern.on_gram else "ovr" if multi else "binary"
        if case == "ovr":
            for name, val in rank_args.items():
                if val is not None:
                    raise NotImplementedError(f"multi-class (one-vs-rest) training runs on one rank from a cold "
                                              f"start: {name} is only supported with two classes")
        if multi:
            Ys = np.stack([np.where(y1 == c, 1.0, -1.0).astype(np.float32) for c in classes])
        else:
            Ys = self._encode(y)[None, :]
        if rank_rows is None and Ys.shape[1] != inp.n:
            raise ValueError(f"len(y) != {inp.what}.shape[0]")
        if case == "binary" and cfg.log_every and progress is None:
            def progress(it, bh, bl, el, hits, misses):  # noqa: E306
                print(f"iter {it}  b_hi {bh:.6g}  b_lo {bl:.6g}  gap {bl - bh:.3g}  "
                      f"{it / max(el, 1e-9):.0f} it/s  hits {hits} misses {misses}", flush=True)
        t0 = time.perf_counter()
        # (the gradients: the training decisions of an input whose model has no predict pass for its own rows)
        p, RC, alphas, infos, setup, self._solver, proba, grads = self._fit_solves(
            inp, y1, Ys, sample_weight, probability, probability_seed, comm, resume, progress, rank_rows,
            keep=case == "binary", want_grads=not inp.train_pass)
        self.wall_time_ = time.perf_counter() - t0
        self._publish(np.stack(alphas).astype(np.float32), Ys, RC, infos, inp, p, setup, grads, y1,
                      partitioned=rank_rows is not None)
        self._publish_proba(proba)
        self._warn_max_iter(case, infos)
        return self

    # the text of each case's max_iter warning; the working-set rounds alone leave the reference's trajectory, so
    # the RBF cases warn only after rounds ran
    _MAX_ITER = {
        "binary": "stopped at max_iter with gap {gap:.3g} > 2 eps: an unconverged working-set model differs from the "
                  "reference's pair-at-a-time iterate at the same cap; raise max_iter to converge, or solver='smo' "
                  "for the reference's trajectory (engines='all' when the Gram is not resident)",
        "ovr": "a one-vs-rest machine stopped at max_iter before its gap closed: raise max_iter to converge",
        "gram": "stopped at max_iter before the gap closed: raise max_iter to converge",
    }

    def _warn_max_iter(self, case: str, infos: list) -> None:
        """called by fit(): the warning points at fit's caller"""
        if any(i["status"] == 2 and (case == "gram" or i.get("outer", 0) > 0) for i in infos):
            import warnings

            warnings.warn(self._MAX_ITER[case].format(gap=infos[0]["b_lo"] - infos[0]["b_hi"]), RuntimeWarning,
                          stacklevel=3)

    def _publish(self, A: np.ndarray, Ys: np.ndarray, RC, infos: list, inp, p, setup, grads, y: np.ndarray,
                 partitioned: bool) -> None:
        """The fitted attributes of the machines' alphas A (k, n) under the labels Ys (k, n) and the row bounds RC
        ((k, n) or None), trained on the input ``inp`` with the caller's labels ``y``; k = 1: the scalar and 1-D
        forms (and ``classes_`` as _encode set it).  ``grads``: the solves' gradients, of an input without a
        predict pass for its own rows; ``partitioned``: this rank holds a part of X — no rows, no support set."""
        multi = self._multi = len(Ys) > 1
        kind, dev = self.config.device_kind()
        self.device_ = f"{kind}:{dev}" if kind == "cuda" else "cpu"
        if setup is not None:
            self.setup_info_ = setup
        self._kgamma = p.gamma  # a spec's gamma as the solver built the Gram with it
        self.gamma_ = inp.published_gamma(p.gamma)
        self.n_features_in_ = inp.shape[1]
        self._model = self._gpu = self._rows_cache = None
        if multi:
            self.classes_ = np.unique(y)
        _publish_solves(self, infos, multi=multi)
        self.alpha_ = A if multi else A[0]
        self.row_C_ = RC if (multi or RC is None) else RC[0]
        bound = RC if RC is not None else np.float32(self.config.C)
        self.n_bounded_ = None if partitioned else int(np.sum((A == bound) & (A > 0)))
        self._Ys = Ys
        # (_y_train: what train_accuracy compares with)
        self._X_train, self._y_train = (None, None) if partitioned else (inp.kept_rows(), y if multi else Ys[0])
        if partitioned:
            return
        self._coef = (A * Ys).astype(np.float32)  # (k, n): the dense coefficients gram_rows_dot reads
        self.support_ = np.nonzero((A > 0).any(axis=0))[0]
        if self._X_train is not None:
            self.support_vectors_ = self._X_train[self.support_]
        else:
            self.__dict__.pop("support_vectors_", None)
        self.dual_coef_ = self._coef[:, self.support_] if multi else self._coef[0, self.support_]
        self.n_support_ = int(len(self.support_))
        if grads is not None:  # the training decisions f + y - b (no predict pass): train_accuracy()
            b = np.atleast_1d(np.asarray(self.b_, dtype=np.float64))
            self._train_dec = np.stack([(grads[c].astype(np.float64) + Ys[c] - b[c]).astype(np.float32)
                                        for c in range(len(Ys))])

    # ------------------------------------------------------------------ cross-validation
    @staticmethod
    def cv_folds(n: int, cv: int = 5, seed: int = 0) -> list:
        """The folds of cross_val_decision: ``np.random.default_rng(seed).permutation(n)`` split by
        ``np.array_split`` into ``cv`` near-equal parts (fold k = the k-th part's row indices)."""
        if not 2 <= cv <= n:
            raise ValueError("cv must be in [2, n]")
        return np.array_split(np.random.default_rng(seed).permutation(n), cv)

    def cross_val_decision(self, X, y, cv: int = 5, seed: int = 0, sample_weight=None) -> np.ndarray:
        """Out-of-fold decision values (n,) of a binary problem: fold k's rows get the decision of the model
        trained with their weights zeroed (C_i = 0: alpha_i stays 0, the row is out of the problem).  On the
        GPU one solver, one setup() and one resident Gram serve the ``cv`` solves: a held-out row's gradient
        entry f_i = sum_j alpha_j y_j K_ij - y_i is kept by every round's f update, so its decision value is
        f_i + y_i - b, read from the solver's gradient — no sub-Gram, no second upload, no predict pass.
        Folds: ``cv_folds(n, cv, seed)``.  ``class_weight='balanced'`` is computed on all n rows.  Settings
        resolve as for a weighted fit.  ``cv_stats_``: the per-fold solve dicts.  kernel="precomputed": X is the
        (n, n) Gram, uploaded once for the ``cv`` solves."""
        X = _train_input(self.config, X)
        y1 = _as_1d(y)
        if len(np.unique(y1)) != 2:
            raise ValueError("cross_val_decision is binary: y needs two classes")
        ys = self._encode(y)
        n, d = X.shape
        if ys.shape[0] != n:
            raise ValueError("len(y) != X.shape[0]")
        p = self.config.to_native(d)
        W = self._weights(y1, ys[None, :], sample_weight)
        self.config.weighted_params(p)
        t0 = time.perf_counter()
        dec, folds, _, _, _, stats, setup, _, _ = self._cv_solves(X, ys[None, :], W, p, cv, seed)
        if setup is not None:
            self.cv_setup_info_ = setup
        self.cv_wall_time_ = time.perf_counter() - t0
        self.cv_stats_ = stats[0]
        self.cv_folds_ = folds
        return dec[0]

    def cross_val_score(self, X, y, cv: int = 5, seed: int = 0, sample_weight=None) -> float:
        """accuracy of the signs of cross_val_decision (>= 0 -> the positive class)"""
        dec = self.cross_val_decision(X, y, cv, seed, sample_weight)
        ys = self._encode(y)
        return float(np.mean(np.where(dec < 0, -1.0, 1.0) == ys))

    # ------------------------------------------------------------------ model
    def to_model(self):
        C = load()
        kern = self._kernel()
        if not kern.has_file:
            raise NotImplementedError("kernel='precomputed' has no model file (there are no rows to write): keep "
                                      "support_, dual_coef_, intercept_ and probA_ / probB_")
        if self._model is None and self._multi:
            try:
                cls = np.asarray(self.classes_, dtype=np.float32)
                self._file_classes = bool(np.array_equal(cls.astype(self.classes_.dtype), self.classes_))
            except (TypeError, ValueError):
                self._file_classes = False
            if not self._file_classes:  # the predictors need only the columns' order
                cls = np.arange(len(self.classes_), dtype=np.float32)
            self._model = _stamp_kernel(C.make_multi_model(self._X_train, cls, self.alpha_, self._Ys, self.b_,
                                                           self._model_gamma()), kern.spec)
        if self._model is None:
            if self._X_train is None:
                raise RuntimeError("to_model() needs the full training set on this rank")
            self._model = _stamp_kernel(C.make_model(self._X_train, self._y_train, self.alpha_, self.b_,
                                                     self._model_gamma()), kern.spec)
        return self._model

    def save(self, path: str, precision: int = 9, legacy: bool = False) -> None:
        """Write the reference text model (gamma, b, then alpha,y,x... per SV);
        after a multi-class fit the one-vs-rest format ("dpsvm-ovr k nsv d",
        classes, gamma, b_0..b_k-1, then the k coefficients and x per SV)."""
        if legacy and self._kernel().spec is not None:
            raise ValueError("the legacy format holds an RBF machine")
        if self._multi:
            if legacy:
                raise ValueError("the legacy format holds one binary machine")
            model = self.to_model()
            if not self._file_classes:
                raise ValueError("the multi-class model file holds numeric class labels exactly representable in "
                                 "float32")
            load().write_multi_model(path, model, precision)
        else:
            load().write_model(path, self.to_model(), precision, legacy)
        _write_platt(path, getattr(self, "probA_", None), getattr(self, "probB_", None))

    # ------------------------------------------------------------------ predict
    def decision_function(self, X, predict_chunk_rows=None) -> np.ndarray:
        """sum_sv alpha y K(sv, x) - b  (svmTrain.cu:646-652).  ``predict_chunk_rows`` (here and in predict,
        predict_proba, score): a kernel-spec model's test rows per chunk of K(test, SV); default: as many as keep
        that scratch within 1 GiB.  The other kernels ignore it."""
        return self._decision(X, predict_chunk_rows=predict_chunk_rows)

    def predict(self, X, predict_chunk_rows=None) -> np.ndarray:
        dec = self.decision_function(X, predict_chunk_rows)
        if self._multi:
            return self.classes_[np.argmax(dec, axis=1)]  # ties: the lowest class index
        return self._decode(np.where(dec < 0, -1.0, 1.0))  # d >= 0 -> +1 (svmTrain.cu:654-657)

    def predict_proba(self, X, predict_chunk_rows=None) -> np.ndarray:
        """(n, k) float32 class probabilities, columns in the order of ``classes_``, after
        ``fit(probability=cv)``: machine c's Platt sigmoid p = 1 / (1 + exp(probA_ d + probB_)) of its decision
        value; two classes: [1 - p, p] with p = P(classes_[-1]); more: the k values divided by their sum (a row
        whose sum is 0: 1 / k each).  On the GPU the sigmoids run on the decision GEMM's output before its
        download.  ``predict`` stays the sign / the argmax of the decision values."""
        return self._predict_proba(X, predict_chunk_rows,
                                   "predict_proba needs fit(probability=cv): this model has no Platt sigmoids")

    def score(self, X, y, predict_chunk_rows=None) -> float:
        yy = _as_1d(y)
        return float(np.mean(self.predict(X, predict_chunk_rows) == yy))

    def train_accuracy(self) -> float:
        """Training accuracy computed on device (distributed across ranks); kernel="precomputed": from the
        solver's gradient, sign(f + y - b) per machine."""
        if self._kernel().on_gram:
            dec = self._train_dec
            if self._multi:
                return float(np.mean(self.classes_[np.argmax(dec, axis=0)] == self._y_train))
            return float(np.mean(np.where(dec[0] < 0, -1.0, 1.0) == self._y_train))
        if self._multi:
            return self.score(self._X_train, self._y_train)  # the multi-output predictor
        if getattr(self, "_solver", None) is not None:
            return float(self._solver.train_accuracy(self.alpha_, self.b_))
        return self.score(self._X_train, self._y_train)

    def get_params(self, deep: bool = True) -> dict:
        return _config_params(self)


class _Loaded(_Predicts):
    """What the loaded models share: the predictor holder, the Platt sidecar's sigmoids, the model's scalars."""

    def __init__(self, model, device: str = "auto", platt=None):
        self.model = model
        self.device = device
        self._check_device()
        self.probA_, self.probB_ = platt if platt is not None else (None, None)  # the sidecar's sigmoids

    def predict_proba(self, X, predict_chunk_rows=None) -> np.ndarray:
        """SVC.predict_proba on the sigmoids read from the model file's ``.platt`` sidecar"""
        return self._predict_proba(X, predict_chunk_rows, "predict_proba needs the model file's .platt sidecar (a "
                                   "model saved after fit(probability=cv))")

    @property
    def gamma(self) -> float:
        return self.model.gamma

    @property
    def b(self):
        return self.model.b

    @property
    def n_support(self) -> int:
        return self.model.nsv

    def _device(self) -> str:
        return self.device

    def _native_model(self):
        return self.model


class LoadedModel(_Loaded):
    """A model read from a reference-format file (svmTest path)."""

    def decision_function(self, X, predict_chunk_rows=None) -> np.ndarray:
        return self._decision(X, predict_chunk_rows=predict_chunk_rows)

    def predict(self, X, predict_chunk_rows=None) -> np.ndarray:
        return np.where(self.decision_function(X, predict_chunk_rows) < 0, -1.0, 1.0).astype(np.float32)

    def score(self, X, y, predict_chunk_rows=None) -> float:
        return float(np.mean(self.predict(X, predict_chunk_rows) == np.where(_as_1d(y) > 0, 1.0, -1.0)))


class LoadedMultiModel(_Loaded):
    """A one-vs-rest model read from a multi-class model file."""

    _multi = True

    def __init__(self, model, device: str = "auto", platt=None):
        super().__init__(model, device, platt)
        self.classes_ = np.asarray(model.classes)

    def decision_function(self, X, predict_chunk_rows=None) -> np.ndarray:
        return self._decision(X, predict_chunk_rows=predict_chunk_rows)

    def predict(self, X, predict_chunk_rows=None) -> np.ndarray:
        return self.classes_[np.argmax(self.decision_function(X, predict_chunk_rows), axis=1)]

    def score(self, X, y, predict_chunk_rows=None) -> float:
        return float(np.mean(self.predict(X, predict_chunk_rows) == _as_1d(y)))


def load_model(path: str, device: str = "auto", legacy: bool = False):
    """A LoadedModel, or a LoadedMultiModel for a multi-class (one-vs-rest) file; with the Platt sigmoids of the
    ``path + ".platt"`` sidecar when there is one (``predict_proba``)."""
    C = load()
    if not legacy and C.is_multi_model(path):
        model = C.read_multi_model(path)
        return LoadedMultiModel(model, device, _read_platt(path, model.k))
    return LoadedModel(C.read_model(path, legacy), device, _read_platt(path, 1))
