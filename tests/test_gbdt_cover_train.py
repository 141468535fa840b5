"""``train --model gbdt --gbdt-cover``: the saved model carries node covers over the real
standardized training rows, the deployed engine then serves ``tree_path`` with no background file,
and without the flag the model file is byte for byte what it was."""
import json
import os

import numpy as np
import pytest

from fraud_detection_amd import train
from fraud_detection_amd.config import Settings
from fraud_detection_amd.ops import gbdt as gb


def test_train_stores_cover_and_engine_serves_tree_path(tmp_path, monkeypatch):
    from fraud_detection_amd.data.synthetic import reference_frame
    from fraud_detection_amd.serve.engine import TreeInferenceEngine
    import fraud_detection_amd.models.gbdt as mg

    df = reference_frame(3000, seed=5)
    csv = tmp_path / "cc.csv"
    df.to_csv(csv, index=False)
    monkeypatch.setenv("DATA_CSV", str(csv))
    monkeypatch.setenv("MLFLOW_TRACKING_URI", str(tmp_path / "mlruns"))
    monkeypatch.setenv("MLFLOW_AUC_THRESHOLD", "0.0")
    orig = gb.GBDTParams
    monkeypatch.setattr(mg.gb, "GBDTParams", lambda **kw: orig(**{"n_estimators": 4, "max_depth": 3, "max_bin": 16, **kw}))
    run = lambda d, **kw: train.run(Settings.load(), cv_folds=0, model_dir=str(tmp_path / d), verbose=False, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="needs --model gbdt"):
        run("x", model_type="logistic", gbdt_cover="count")
    with pytest.raises(ValueError, match="hessian or count"):
        run("x", model_type="gbdt", gbdt_cover="gain")
    plain = run("plain", model_type="gbdt")
    out = run("cover", model_type="gbdt", gbdt_cover="count")
    assert "gbdt_cover" not in plain and out["gbdt_cover"]["kind"] == "count"
    a = json.loads((tmp_path / "plain" / "xgb_model.json").read_text())
    b = json.loads((tmp_path / "cover" / "xgb_model.json").read_text())
    assert "cover" not in a and b["cover_kind"] == "count"
    cover = np.asarray(b.pop("cover"))
    b.pop("cover_kind")
    assert json.dumps(a) == json.dumps(b)  # the same fit; the cover is the file's only difference
    assert np.all(cover[:, 1] == out["gbdt_cover"]["rows"])  # every real training row, no SMOTE sample
    os.remove(tmp_path / "cover" / "shap_background.npy")
    eng = TreeInferenceEngine.from_paths(str(tmp_path / "cover" / "xgb_model.json"), device="cpu")
    assert not eng.has_background
    X = df.drop(columns=["Class"]).to_numpy(np.float32)[:5]
    ex = eng.explain(X, "tree_path")
    assert ex.method == "tree_path" and ex.phi.shape == (5, X.shape[1])
    np.testing.assert_allclose(ex.phi.sum(1), ex.logit - ex.base_value, rtol=0, atol=1e-6)
    plain_eng = TreeInferenceEngine.from_paths(str(tmp_path / "plain" / "xgb_model.json"), device="cpu")
    with pytest.raises(ValueError, match="node covers"):
        plain_eng.explain(X, "tree_path")
