"""Linear, polynomial and sigmoid kernels end to end on the GPU (docs/DESIGN.md §21): the Gram built from the rows
straight into the solver's lines (setup_rows_gram), then a precomputed-kernel solve; decisions from K(test, SV)
built per chunk of test rows — against kernel="precomputed" on ops.kernel_gram(X) bit for bit, against
scikit-learn's own kernels (tests/data/sklearn_named_kernels.json) and against the CPU fit.

Bounds against scikit-learn and the CPU fit: 10 x the setting's recorded ``dev`` (scikit-learn at tol 1e-3 against
tol 1e-7), on the decisions and on the intercept.
"""
import numpy as np
import pytest
import torch

from test_named_kernels_cpu import bits, check_against_fixture, decisions, fit, load_fixture, make, spec_of

pytestmark = pytest.mark.gpu

NOTE = "precomputed Gram: general diagonal, one block"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def gpu_fits(fx):
    """one GPU fit per fixture setting, shared by the tests below"""
    return [fit(make(s["kind"], spec_of(s), s["gamma"], device="cuda"), s["kind"], fx["X"][:fx["n"]], fx)
            for s in fx["settings"]]


def op_gram(X, spec, gamma) -> torch.Tensor:
    from dpsvm_amd.ops import kernels as ops

    return ops.kernel_gram(torch.tensor(X, dtype=torch.float32, device="cuda"), None, kernel=spec, gamma=gamma)


def check_setup(m, name: str) -> None:
    si = m.setup_info_
    assert si["kernel"] == name and si["gram"] == "precomputed"
    assert si["iteration"] == "ws-dense" and si["ws_rows"] == "gram" and si["ws_blocks"] == 1
    assert NOTE in si["engine_note"] and si["t_gram_build"] > 0
    for st in (m.stats_ if isinstance(m.stats_, list) else [m.stats_]):
        assert st["t_gram"] == 0 and st["gram_reused"] is True


@pytest.mark.parametrize("k", range(5))
def test_spec_fit_equals_precomputed_on_the_ops_gram(fx, gpu_fits, k):
    s, a = fx["settings"][k], gpu_fits[k]
    n, spec, gamma = fx["n"], spec_of(s), s["gamma"]
    b = fit(make(s["kind"], "precomputed", None, device="cuda"), s["kind"], op_gram(fx["X"][:n], spec, gamma), fx)
    np.testing.assert_array_equal(bits(a.alpha_), bits(b.alpha_))
    assert np.float32(a.b_).view(np.uint32) == np.float32(b.b_).view(np.uint32)
    assert a.converged_ and a.status_ == 1
    check_setup(a, s["kernel"])
    assert a.support_vectors_.shape == (a.n_support_, fx["X"].shape[1]) and a.n_features_in_ == fx["X"].shape[1]
    assert a.gamma_ is None if s["kernel"] == "linear" else a.gamma_ == pytest.approx(gamma)


@pytest.mark.parametrize("k", range(5))
def test_gpu_matches_sklearn_and_cpu(fx, gpu_fits, k):
    s, m = fx["settings"][k], gpu_fits[k]
    n = fx["n"]
    check_against_fixture(m, s, fx, "gpu")
    ref = fit(make(s["kind"], spec_of(s), s["gamma"], device="cpu"), s["kind"], fx["X"][:n], fx)
    tol = 10.0 * s["dev"]
    e = [float(np.max(np.abs(decisions(m, s["kind"], X) - decisions(ref, s["kind"], X))))
         for X in (fx["X"][:n], fx["X"][n:])]
    e_b = abs(float(m.intercept_) - float(ref.intercept_))
    print(f"gpu vs cpu {s['kind']} {s['kernel']}: max |d decision| {e[0]:.3g} / {e[1]:.3g} |d intercept| {e_b:.3g} "
          f"(bound {tol:.3g})")
    assert max(e) < tol and e_b < tol


def test_odd_n_three_class_weighted_probability(fx):
    """n = 601 (no multiple of anything), three classes, sample weights, probability folds: every machine's alpha
    and b, the sigmoids and the probabilities bit-equal to the precomputed fit on the op's Gram"""
    from dpsvm_amd import Poly

    n, spec, gamma = 601, Poly(3, 1.0), 0.1
    X = fx["X"][:n]
    y3 = np.where(X[:, 0] < -0.3, 0, np.where(X[:, 0] < 0.3, 1, 2))
    w = 0.5 + (np.arange(n) % 4) * 0.5
    a = make("svc", spec, gamma, device="cuda").fit(X, y3, sample_weight=w, probability=3)
    K = op_gram(X, spec, gamma)
    b = make("svc", "precomputed", None, device="cuda").fit(K, y3, sample_weight=w, probability=3)
    assert a.alpha_.shape == (3, n)
    np.testing.assert_array_equal(bits(a.alpha_), bits(b.alpha_))
    np.testing.assert_array_equal(bits(a.b_), bits(b.b_))
    np.testing.assert_array_equal(a.probA_, b.probA_)
    np.testing.assert_array_equal(a.probB_, b.probB_)
    check_setup(a, "poly")
    assert len(a.stats_) == 3 and a.train_accuracy() == b.train_accuracy()
    # chunked prediction: 300 test rows in chunks of 128 (two full, one partial) against one chunk
    Xt = np.ascontiguousarray(np.concatenate([fx["X"][601:], fx["X"][:101]]))
    assert len(Xt) == 300
    d1, d3 = a.decision_function(Xt), a.decision_function(Xt, predict_chunk_rows=128)
    assert d1.shape == (300, 3)
    np.testing.assert_array_equal(bits(d1), bits(d3))
    from dpsvm_amd.ops import kernels as ops

    Kt = ops.kernel_gram(torch.from_numpy(Xt).cuda(), torch.tensor(X, dtype=torch.float32, device="cuda"), kernel=spec,
                         gamma=gamma)
    np.testing.assert_array_equal(bits(d1), bits(b.decision_function(Kt)))
    p1, p3 = a.predict_proba(Xt), a.predict_proba(Xt, predict_chunk_rows=128)
    np.testing.assert_array_equal(bits(p1), bits(p3))
    assert p1.shape == (300, 3) and float(np.max(np.abs(p1.sum(axis=1) - 1.0))) < 1e-5
    np.testing.assert_array_equal(a.predict(Xt, predict_chunk_rows=128), a.classes_[np.argmax(d1, axis=1)])


def test_device_rows_cross_validation_and_nu_path(fx):
    """X as a float32 tensor on the device is read in place; cross_val_decision and nu_path run on the built Gram"""
    from dpsvm_amd import Poly

    n, spec, gamma = 600, Poly(2, 1.0), 0.1
    X, y = fx["X"][:n], fx["y"][:n]
    Xd = torch.tensor(X, dtype=torch.float32, device="cuda")
    a = make("svc", spec, gamma, device="cuda").fit(X, y)
    b = make("svc", spec, gamma, device="cuda").fit(Xd, y)
    np.testing.assert_array_equal(bits(a.alpha_), bits(b.alpha_))
    assert a.b_ == b.b_ and np.array_equal(b.support_vectors_, X[b.support_])
    K = op_gram(X, spec, gamma)
    np.testing.assert_array_equal(
        bits(make("svc", spec, gamma, device="cuda").cross_val_decision(X, y, cv=3)),
        bits(make("svc", "precomputed", None, device="cuda").cross_val_decision(K, y, cv=3)))
    oa, ob = make("oneclass", spec, gamma, device="cuda"), make("oneclass", "precomputed", None, device="cuda")
    pa, pb = oa.nu_path(X, [0.1, 0.2, 0.4]), ob.nu_path(K, [0.1, 0.2, 0.4])
    assert pa == pb
    np.testing.assert_array_equal(bits(oa.path_alpha_), bits(ob.path_alpha_))
    assert [st["gram_reused"] for st in oa.path_stats_] == [True, True, True]
    assert all(st["t_gram"] == 0 for st in oa.path_stats_) and oa.path_setup_info_["kernel"] == "poly"
    assert oa.path_setup_info_["t_gram_build"] > 0


@pytest.mark.parametrize("k", range(5))
def test_model_files(fx, gpu_fits, tmp_path, k):
    """saved on the GPU: loaded on the GPU the decisions are bit-equal, loaded on the CPU within the fixture bound"""
    from dpsvm_amd import load_model, load_one_class, load_svr

    s, m = fx["settings"][k], gpu_fits[k]
    Xt = fx["X"][fx["n"]:]
    path = str(tmp_path / "m.txt")
    m.save(path)
    assert open(path).readline().startswith(f"dpsvm-kernel {s['kernel']} ")
    loader = {"svc": load_model, "svr": load_svr, "oneclass": load_one_class}[s["kind"]]
    d = decisions(m, s["kind"], Xt)
    np.testing.assert_array_equal(bits(decisions(loader(path, device="cuda"), s["kind"], Xt)), bits(d))
    e = float(np.max(np.abs(decisions(loader(path, device="cpu"), s["kind"], Xt) - d)))
    print(f"{s['kind']} {s['kernel']}: GPU model on the CPU, max |d decision| {e:.3g} (bound {10 * s['dev']:.3g})")
    assert e < 10.0 * s["dev"]


def test_one_vs_rest_model_file(fx, tmp_path):
    from dpsvm_amd import Poly, load_model

    n = 300
    X, Xt = fx["X"][:n], fx["X"][600:700]
    y3 = np.where(X[:, 0] < -0.3, 0, np.where(X[:, 0] < 0.3, 1, 2))
    m = make("svc", Poly(2, 1.0), 0.1, device="cuda").fit(X, y3, probability=3)
    path = str(tmp_path / "ovr.txt")
    m.save(path)
    back = load_model(path, device="cuda")
    np.testing.assert_array_equal(bits(back.decision_function(Xt)), bits(m.decision_function(Xt)))
    np.testing.assert_array_equal(bits(back.predict_proba(Xt)), bits(m.predict_proba(Xt)))
    np.testing.assert_array_equal(back.predict(Xt), m.predict(Xt))


def test_fit_memory_is_one_gram(fx):
    """n = 2,048: what the solver holds after setup plus torch's peak (X on the device) stays below 1.5 Grams —
    a second copy of the Gram (the caller's, as kernel="precomputed" needs) would make it 2"""
    from dpsvm_amd import Poly

    n, d = 2048, 20
    rng = np.random.default_rng(9)
    X = rng.uniform(-0.875, 0.875, size=(n, d)).astype(np.float32)
    y = np.where(X[:, 0] + 0.5 * X[:, 1] > 0, 1.0, -1.0)
    Xd = torch.from_numpy(X).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m = make("svc", Poly(3, 1.0), 0.1, device="cuda").fit(Xd, y)
    peak = torch.cuda.max_memory_allocated() - base + Xd.numel() * 4
    held = int(m.setup_info_["bytes_device"])
    gram = n * n * 4  # the lines' stride is >= n
    print(f"bytes_device {held} + torch peak {peak} = {(held + peak) / gram:.3f} Grams")
    assert m.converged_ and gram <= held and held + peak < 1.5 * gram


def test_negative_diagonal_and_refusals_gpu(fx):
    from dpsvm_amd import Poly, Sigmoid

    n = 200
    X, y = fx["X"][:n], fx["y"][:n]
    with pytest.raises(ValueError, match="invalid Gram: diagonal"):
        make("svc", Sigmoid(-5.0), 0.02, device="cuda").fit(X * np.float32(1e-3), y)
    with pytest.raises(NotImplementedError, match="ws_blocks"):
        make("svc", Poly(3, 1.0), 0.1, device="cuda", ws_blocks=4)
    for kw in (dict(comm=object()), dict(resume="ck.bin"), dict(rank_rows=10)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            make("svc", Poly(3, 1.0), 0.1, device="cuda").fit(X, y, **kw)
    m = make("svc", Poly(3, 1.0), 0.1, device="cuda").fit(X, y)  # the solver is usable after the refusals
    assert m.converged_
