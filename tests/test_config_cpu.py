"""SVCConfig.to_native: every field that reaches SolverParams arrives as the mapped value (the enum
tables are spelled out here, not imported), the special cases, the refusals; and the device strings
of SVCConfig.device_kind and load_model."""
import numpy as np
import pytest

from dpsvm_amd.models.svc import SVC, SVCConfig, load_model

AUTO_ON_OFF = {"auto": 0, "on": 1, "off": 2}
# SVCConfig field -> (SolverParams attribute, {string: native value})
ENUMS = {
    "x_mode": ("x_mode", {"auto": 0, "replicated": 1, "partitioned": 2}),
    "exchange": ("exchange", {"auto": 0, "allreduce": 1, "peer": 2}),
    "persist": ("persist", {"auto": 0, "off": 1, "on": 2}),
    "dp": ("dp_policy", {"auto": 0, "shard": 1, "replicate": 2}),
    "cache_engine": ("cache_engine", {"fused": 0, "chain": 1}),
    "engines": ("engines", {"production": 0, "all": 1}),
    "xch_mem": ("xch_mem", {"auto": 0, "uncached": 1, "coarse": 2}),
    "solver": ("solver", {"auto": 0, "smo": 1, "ws": 2}),
    "ws_recompute": ("ws_recompute", AUTO_ON_OFF),
    "eta": ("eta", {"x": 0, "gram": 1}),
    "gram": ("gram_precision", {"auto": 0, "f32": 1, "split": 2}),
    "gram_adapt": ("gram_adapt", AUTO_ON_OFF),
}
# SVCConfig field -> (a non-default value, SolverParams attribute, the native value)
PLAIN = {
    "C": (3.5, "C", 3.5),
    "gamma": (0.375, "gamma", 0.375),
    "eps": (0.0625, "eps", 0.0625),
    "max_iter": (1234, "max_iter", 1234),
    "tau": (2.0 ** -30, "tau", 2.0 ** -30),
    "cache_lines": (77, "cache_lines", 77),
    "cache_mb": (12.5, "cache_mb", 12.5),
    "cache_frac": (0.5, "cache_frac", 0.5),
    "host_cache_lines": (9, "host_cache_lines", 9),
    "spec_rows": (5, "spec_rows", 5),
    "graph_block": (32, "graph_block", 32),
    "use_graph": (False, "use_graph", False),
    "log_every": (10, "log_every", 10),
    "checkpoint_path": ("ck.bin", "checkpoint_path", "ck.bin"),
    "checkpoint_every": (500, "checkpoint_every", 500),
    "verbose": (True, "verbose", True),
    "force_collectives": (True, "force_collectives", True),
    "persist_block": (512, "persist_block", 512),
    "force_cache": (True, "force_cache", True),
    "cache_groups": (128, "cache_groups", 128),
    "rows_per_group": (512, "rows_per_group", 512),
    "xch_poll_batch": (3, "xch_poll_batch", 3),
    "xch_sleep": (2, "xch_sleep", 2),
    "xch_stride": (8, "xch_stride", 8),
    "xch_timeout_s": (7.5, "xch_timeout_s", 7.5),
    "watchdog_s": (60.0, "watchdog_s", 60.0),
    "census_groups": (4, "census_groups", 4),
    "verify_ranks": (False, "verify_ranks", False),
    "ws_size": (96, "ws_size", 96),
    "ws_new": (48, "ws_new", 48),
    "ws_rel": (0.25, "ws_rel", 0.25),
    "ws_blocks": (4, "ws_blocks", 4),
    "ws_inner": (100, "ws_inner", 100),
    "ws_wss": (2, "ws_wss", 2),
    "ws_block": (4, "ws_block", 4),
    "ws_t_halve": (0.75, "ws_t_halve", 0.75),
    "ws_clip_fallback": (False, "ws_clip_fallback", 0),
    "gram_cold_tau": (2.0 ** -20, "gram_cold_tau", 2.0 ** -20),
}
NOT_NATIVE = {"device", "shrink", "class_weight"}  # resolved by the estimator


def test_every_field_is_covered():
    import dataclasses

    fields = {f.name for f in dataclasses.fields(SVCConfig)}
    assert fields == set(PLAIN) | set(ENUMS) | {"clip"} | NOT_NATIVE


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_plain_field_reaches_native(name):
    value, attr, native = PLAIN[name]
    assert getattr(SVCConfig(), name) != value
    got = getattr(SVCConfig(**{name: value}).to_native(8), attr)
    assert got == native and type(got) is type(native)


@pytest.mark.parametrize("name", sorted(ENUMS))
def test_enum_field_maps_by_its_table(name):
    attr, table = ENUMS[name]
    for text, native in table.items():
        assert getattr(SVCConfig(**{name: text}).to_native(8), attr) == native
    with pytest.raises(ValueError):
        SVCConfig(**{name: "no-such-value"}).to_native(8)


def test_clip(C):
    assert SVCConfig(clip="independent").to_native(8).clip == C.ClipMode.independent
    assert SVCConfig(clip="box").to_native(8).clip == C.ClipMode.box
    with pytest.raises(ValueError):
        SVCConfig(clip="no-such-value").to_native(8)


def test_special_cases():
    p = SVCConfig().to_native(8)
    assert p.gamma == np.float32(1.0 / 8) and p.checkpoint_path == "" and p.ws_clip_fallback == 1
    assert SVCConfig(gamma=None).to_native(5).gamma == np.float32(1.0 / 5)
    for bad in (dict(rows_per_group=100), dict(C=0), dict(C=-1.0)):
        with pytest.raises(ValueError):
            SVCConfig(**bad).to_native(8)


def test_device_kind():
    assert SVCConfig(device="cpu").device_kind() == ("cpu", 0)
    assert SVCConfig(device="cuda").device_kind() == ("cuda", 0)
    assert SVCConfig(device="cuda:3").device_kind() == ("cuda", 3)
    assert SVCConfig(device="auto").device_kind() in (("cpu", 0), ("cuda", 0))
    with pytest.raises(ValueError):
        SVCConfig(device="tpu").device_kind()


def test_load_model_rejects_an_unknown_device(tmp_path):
    rng = np.random.default_rng(0)
    y = np.where(rng.random(60) < 0.5, -1.0, 1.0)
    X = (rng.standard_normal((60, 4)) + y[:, None]).astype(np.float32)
    clf = SVC(C=1.0, gamma=0.25, device="cpu").fit(X, y)
    path = str(tmp_path / "binary.model")
    clf.save(path)
    loaded = load_model(path, device="cpu")
    assert np.array_equal(loaded.decision_function(X), clf.decision_function(X))
    with pytest.raises(ValueError):  # not a silent CPU run
        load_model(path, device="tpu")
