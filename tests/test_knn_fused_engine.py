"""Engine selection with bf16x3f in the set (ops/knn.py knn_engine; no GPU): the name is accepted by
``engine=`` and by FDX_KNN, and ``auto`` picks a two-pass engine -- bf16x3t or its one-launch form --
exactly where it picked bf16x3t before: 8k..16k candidates with at least 4k queries."""
import pytest

from fraud_detection_amd.ops import knn as K


def _auto_before(mq, mc):  # auto's rule before bf16x3f existed
    if mc < (1 << 13):
        return "fp32"
    return "bf16x3t" if mc <= (1 << 14) and mq >= (1 << 12) else "bf16x3r"


def test_the_name_is_accepted(monkeypatch):
    assert K.knn_engine(10, 10, "bf16x3f") == "bf16x3f"
    monkeypatch.setenv("FDX_KNN", "bf16x3f")
    assert K.knn_engine(10, 10) == "bf16x3f" and K.knn_engine(10, 10, "fp32") == "fp32"
    for e in ("fp32", "bf16x3r", "bf16x3t"):
        assert K.knn_engine(13_600, 13_600, e) == e
    with pytest.raises(ValueError):
        K.knn_engine(10, 10, "bf16x3g")


def test_auto_picks_a_two_pass_engine_only_where_it_picked_bf16x3t(monkeypatch):
    monkeypatch.delenv("FDX_KNN", raising=False)
    assert K.knn_engine(10, 4_000) == "fp32" and K.knn_engine(10, 13_600) == "bf16x3r"
    assert K.KNN_TWOPASS_ENGINE in ("bf16x3t", "bf16x3f")
    edges = [1, 10, 4095, 4096, 4097, 8191, 8192, 8193, 13_600, 16_383, 16_384, 16_385, 108_800, 1_000_000]
    for mq in edges:
        for mc in edges:
            got, was = K.knn_engine(mq, mc), _auto_before(mq, mc)
            if was == "bf16x3t":
                assert got == K.KNN_TWOPASS_ENGINE, (mq, mc)
            else:
                assert got == was, (mq, mc)
    assert K.knn_engine(13_600, 13_600) == K.KNN_TWOPASS_ENGINE and K.knn_engine(13_600, 108_800) == "bf16x3r"
