"""The three problem kinds on one X (csrc/include/dpsvm/problem.hpp): which GpuSolver calls each kind serves and
which it refuses, by name; a refused call leaves the solver as it was, an allowed swap call keeps the Gram."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KINDS = {"classification": {}, "epsilon-SVR": dict(problem=1, svr_epsilon=0.1), "one-class": dict(one_class_nu=0.2)}
CALLS = ["set_labels", "set_nu", "set_row_C", "train_accuracy", "decision", "holdout_decisions", "platt_fit",
         "solve_resume"]
SWAPS = ("set_labels", "set_nu", "set_row_C")   # what problem_swapped accounts for
ALLOWED = {"classification": set(CALLS) - {"set_nu"}, "epsilon-SVR": {"set_labels"},
           "one-class": {"set_nu", "decision"}}


@pytest.fixture(scope="module")
def X():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "sklearn_oneclass.json")) as f:
        return np.array(json.load(f)["X"], dtype=np.float32)


@pytest.mark.parametrize("kind", list(KINDS))
def test_problem_kind_serves_and_refuses(C, X, kind):
    n = len(X)
    y = {"classification": np.where(X[:, 0] > 0, 1.0, -1.0), "epsilon-SVR": np.sin(X[:, 0]) + 0.5 * X[:, 1],
         "one-class": np.zeros(n)}[kind].astype(np.float32)
    p = C.SolverParams()
    p.C, p.gamma, p.eps, p.clip, p.solver, p.ws_blocks = 1.0, 0.5, 1e-3, C.ClipMode.box, 2, 1
    for k, v in KINDS[kind].items():
        setattr(p, k, v)
    solver = C.GpuSolver(p, None, 0)
    solver.setup(X, n, y)
    alpha, info = solver.solve()
    assert info["converged"] and not info["gram_reused"]
    assert len(alpha) == (2 * n if kind == "epsilon-SVR" else n)
    f = solver.gradient()
    ck = C.Checkpoint()
    if kind == "classification":   # the solved state: a resume the classifier accepts
        ck.n, ck.d, ck.C, ck.gamma, ck.eps, ck.clip = n, X.shape[1], 1.0, 0.5, 1e-3, 1
        ck.iter, ck.b_hi, ck.b_lo, ck.alpha, ck.f = info["iters"], info["b_hi"], info["b_lo"], alpha, f
    rows = np.arange(5, dtype=np.int32)
    calls = {"set_labels": lambda: solver.set_labels(y), "set_nu": lambda: solver.set_nu(0.2),
             "set_row_C": lambda: solver.set_row_C(np.ones(n, np.float32)),
             "train_accuracy": lambda: solver.train_accuracy(alpha[:n], info["b"]),
             "decision": lambda: solver.decision(alpha[:n], info["b"], X[:7]),
             "holdout_decisions": lambda: solver.holdout_decisions(rows, info["b"], 0),
             "platt_fit": lambda: solver.platt_fit(0), "solve_resume": lambda: solver.solve(ck)}
    for name in CALLS:   # (holdout_decisions comes before platt_fit: the classifier's slot 0 exists)
        ok = name in ALLOWED[kind]
        if ok:
            calls[name]()
        else:
            # a refusal names the kind; the classifier's refusal of set_nu names what it is not
            with pytest.raises(RuntimeError, match="one-class" if kind == "classification" else kind):
                calls[name]()
        if name in SWAPS:
            again, info2 = solver.solve()
            np.testing.assert_array_equal(again, alpha)
            assert info2["gram_reused"] is ok
        if name == "set_row_C" and ok:   # back to the scalar C: resume and per-row C do not combine
            solver.set_row_C(None)
            again, info2 = solver.solve()
            np.testing.assert_array_equal(again, alpha)
            assert info2["gram_reused"]
    again, info2 = solver.solve()   # and nothing above asked to keep the Gram
    np.testing.assert_array_equal(again, alpha)
    assert not info2["gram_reused"]
