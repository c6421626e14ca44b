"""What test_fit_attributes_cpu.py and test_fit_attributes_gpu.py share: the seeded data, the literal table of the
public fitted attributes (``name_``) — each one's type, dtype and shape — and the checks against it.

The table was written down from the behaviour of the commit before the model layer's fit paths were merged into
one; it is the record of what a fit publishes, not a description of the code.  Shapes use n (training rows), d
(features), k (one-vs-rest machines), s (support vectors: len(support_)) and f (probability folds).
"""
import numpy as np

N, D, FOLDS = 96, 6, 3
C_BOUND = 2.0

# ---------------------------------------------------------------------------------------------- the literal table
# every fit of every estimator
COMMON = {
    "converged_": "bool", "device_": "str", "fit_time_": "float", "setup_time_": "float", "wall_time_": "float",
    "status_": "int", "n_features_in_": "int", "n_support_": "int", "support_": "int64[s]",
    "support_vectors_": "float32[s, d]",  # (not with kernel="precomputed": there are no rows to keep)
    "gamma_": "float",                    # (None with kernel="precomputed" and Linear())
}
# one machine: Python scalars and 1-D arrays ...
ONE = {"b_": "float", "intercept_": "float", "n_iter_": "int", "n_rounds_": "int", "stats_": "dict"}
# ... k machines: stacked
MANY = {"b_": "float32[k]", "intercept_": "float32[k]", "n_iter_": "int64[k]", "n_rounds_": "int64[k]",
        "stats_": "list[k]<dict>"}
SVC_ONE = {**ONE, "alpha_": "float32[n]", "dual_coef_": "float32[s]", "classes_": "float32[2]",
           "n_bounded_": "int", "row_C_": "NoneType"}
SVC_MANY = {**MANY, "alpha_": "float32[k, n]", "dual_coef_": "float32[k, s]", "classes_": "int64[k]",
            "n_bounded_": "int", "row_C_": "NoneType"}
WEIGHTED = {False: {"row_C_": "float32[n]"}, True: {"row_C_": "float32[k, n]"}}  # by multi
PROBA_OFF = {"cv_decision_": "NoneType", "platt_stats_": "NoneType", "probA_": "NoneType", "probB_": "NoneType"}
PROBA_ONE = {"cv_decision_": "float32[n]", "cv_folds_": "list[f]<int64[32]>", "cv_stats_": "list[f]<dict>",
             "platt_stats_": "dict", "probA_": "np.float64", "probB_": "np.float64"}
PROBA_MANY = {"cv_decision_": "float32[n, k]", "cv_folds_": "list[f]<int64[32]>",
              "cv_stats_": "list[k]<list[f]<dict>>", "platt_stats_": "list[k]<dict>", "probA_": "float64[k]",
              "probB_": "float64[k]"}
SVR_ONLY = {**ONE, "alpha_": "float32[2, n]", "dual_coef_": "float32[s]", "n_common_": "int",
            "setup_info_": "dict"}
ONE_CLASS_ONLY = {**ONE, "alpha_": "float32[n]", "dual_coef_": "float32[s]", "offset_": "float",
                  "train_decision_": "float32[n]", "setup_info_": "dict"}


def expected(kind: str, kernel: str, multi: bool = False, weights: bool = False, prob: int = 0,
             device: str = "cpu") -> dict:
    """the table of one fit on a fresh estimator; kernel: rbf | precomputed | poly | linear"""
    t = dict(COMMON)
    if kind == "svc":
        t.update(SVC_MANY if multi else SVC_ONE)
        if weights:
            t.update(WEIGHTED[multi])
        t.update((PROBA_MANY if multi else PROBA_ONE) if prob else PROBA_OFF)
        # an RBF fit on the CPU publishes no setup info; a Gram fit does ({"iteration": "cpu", ...}); the GPU always
        if kernel != "rbf" or device != "cpu":
            t["setup_info_"] = "dict"
    else:
        t.update(SVR_ONLY if kind == "svr" else ONE_CLASS_ONLY)
    if kernel == "precomputed":
        del t["support_vectors_"]
    if kernel in ("precomputed", "linear"):
        t["gamma_"] = "NoneType"
    return t


# --------------------------------------------------------------------------------------------------------- data
def data() -> dict:
    rng = np.random.default_rng(7)
    X = rng.standard_normal((N, D)).astype(np.float32)
    w = rng.standard_normal(D)
    y2 = np.where(X @ w + 0.3 * rng.standard_normal(N) > 0, 1.0, -1.0).astype(np.float32)
    y3 = np.digitize(X @ w, [-0.8, 0.8]).astype(np.int64)
    assert set(y2.tolist()) == {-1.0, 1.0} and set(y3.tolist()) == {0, 1, 2}  # every class present
    z = (np.sin(X @ w) + 0.1 * rng.standard_normal(N)).astype(np.float32)
    sw = rng.uniform(0.5, 2.0, N)
    K = X.astype(np.float64) @ X.astype(np.float64).T
    K = (0.5 * (K + K.T)).astype(np.float32)
    K = np.ascontiguousarray(np.triu(K) + np.triu(K, 1).T)  # K = X X^T, symmetric bitwise
    return dict(X=X, y2=y2, y3=y3, z=z, sw=sw, K=K)


def kernel_of(name: str):
    from dpsvm_amd import Linear, Poly

    return {"rbf": "rbf", "precomputed": "precomputed", "poly": Poly(2, 1.0), "linear": Linear()}[name]


def fit(dat, kind: str, kernel: str, multi=False, weights=False, prob=0, device="cpu", est=None):
    """one fit of the matrix (on ``est`` when given: a refit); returns the estimator"""
    from dpsvm_amd import SVC, SVR, OneClassSVM

    train = dat["K"] if kernel == "precomputed" else dat["X"]
    kw = dict(gamma=0.5, device=device, clip="box", kernel=kernel_of(kernel))
    if kind == "svc":
        est = est if est is not None else SVC(C=C_BOUND, **kw)
        return est.fit(train, dat["y3"] if multi else dat["y2"], sample_weight=dat["sw"] if weights else None,
                       probability=prob)
    if kind == "svr":
        return SVR(C=C_BOUND, epsilon=0.05, **kw).fit(train, dat["z"])
    return OneClassSVM(nu=0.3, **kw).fit(train)


# ------------------------------------------------------------------------------------------------------- checks
def describe(v) -> str:
    if isinstance(v, np.ndarray):
        return f"{v.dtype}{list(v.shape)}"
    if isinstance(v, np.generic):
        return f"np.{v.dtype}"
    if isinstance(v, list):
        return f"list[{len(v)}]<{describe(v[0])}>"
    return type(v).__name__


def table(est) -> dict:
    """the public fitted attributes of ``est`` as {name: description}"""
    return {k: describe(v) for k, v in vars(est).items() if k.endswith("_") and not k.startswith("_")}


def resolve(t: dict, est, k: int = 3) -> dict:
    """the literal table with its letters replaced by this fit's sizes"""
    dims = {"n": N, "d": D, "k": k, "s": len(est.support_), "f": FOLDS}
    out = {}
    for name, spec in t.items():
        for letter, val in dims.items():
            spec = spec.replace(f"[{letter}", f"[{val}").replace(f", {letter}", f", {val}")
        out[name] = spec
    return out


def check_table(est, t: dict) -> None:
    got, want = table(est), resolve(t, est)
    assert set(got) == set(want), (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    for name in ("gamma_", "row_C_", "cv_decision_", "platt_stats_", "probA_", "probB_"):
        if want.get(name) == "NoneType":
            assert getattr(est, name) is None
    assert ("setup_info_" in vars(est)) == ("setup_info_" in t)
    assert hasattr(est, "support_vectors_") == ("support_vectors_" in t)


def check_consistency(est, dat, kind: str, multi: bool) -> None:
    """dual_coef_ = (alpha_ * Ys)[..., support_]; n_bounded_ = #{alpha == bound > 0}"""
    a = est.alpha_
    if kind == "svc":
        if multi:
            Ys = np.stack([np.where(dat["y3"] == c, 1.0, -1.0).astype(np.float32) for c in est.classes_])
        else:
            Ys = dat["y2"]
        assert np.array_equal(est.support_, np.nonzero((np.atleast_2d(a) > 0).any(axis=0))[0])
        assert np.array_equal(est.dual_coef_, (a * Ys)[..., est.support_])
        bound = est.row_C_ if est.row_C_ is not None else np.float32(C_BOUND)
        assert est.n_bounded_ == int(np.sum((a == bound) & (a > 0)))
    elif kind == "svr":
        assert np.array_equal(est.dual_coef_, (a[0] - a[1])[est.support_])
    else:
        assert np.array_equal(est.dual_coef_, a[est.support_])
    assert est.n_support_ == len(est.support_)
