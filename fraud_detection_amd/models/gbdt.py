"""Gradient-boosted trees family (the reference's XGBoost path, train_model.py:49-114).

* ``GBDTClassifier`` -- estimator with xgboost.XGBClassifier's parameter names
  (n_estimators, learning_rate, max_depth, reg_lambda, min_child_weight, gamma, max_bin,
  scale_pos_weight, base_score, monotone_constraints, interaction_constraints, reg_alpha,
  max_delta_step) over numpy arrays or torch tensors; device kernels on a GPU
  tensor, the numpy oracle on CPU.  Models serialise to JSON (no pickle).  With node covers
  in the model (``fit(..., record_cover=True)`` or ``compute_cover``) it explains itself without a
  background: ``predict_contribs`` (xgboost's pred_contribs, [n, d + 1]) and
  ``predict_interactions`` (pred_interactions, [n, d + 1, d + 1]).
* ``GBDTPipeline`` -- the reference's per-fold recipe on device: StandardScaler fit on the
  fold's rows -> SMOTE (MFMA k-NN + Philox interpolation, fp32 rows) -> boosting -> exact AUC.
  ``scale_pos_weight="auto"`` (default) is neg/pos of the rows the trees are fit on, i.e. AFTER
  SMOTE (= 1 at sampling_ratio 1): the reference computes neg/pos BEFORE SMOTE
  (train_model.py:52-54) and applies it to the SMOTE-balanced rows (:77), compensating the class
  imbalance twice (AUC 0.9467 < 0.95 on the bench data, profiles/r2_s4b).
  ``scale_pos_weight="reference"`` reproduces that pre-SMOTE value on purpose; a number is used
  as given.
"""
from __future__ import annotations

import json
import os
import time
from dataclasses import dataclass, field

import numpy as np
import torch

from ..ops import gbdt as gb
from ..ops import knn as knn_ops
from ..ops import metrics as metric_ops
from ..ops import scaler as scaler_ops
from ..ops.layout import NCOLS
from .pipeline import TrainConfig, global_smote_slices

MODEL_FILE = "xgb_model.json"
JOBLIB_FILE = "xgb_model.joblib"  # the reference's artifact name (train_model.py:113)
_PARAM_FIELDS = frozenset(gb.GBDTParams.__dataclass_fields__)


def _as_tensor(X, device=None, dtype=torch.float32) -> torch.Tensor:
    t = X if isinstance(X, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(X, dtype=np.float32)))
    if device is not None:
        t = t.to(device)
    return t.to(dtype).contiguous() if t.dtype != dtype or not t.is_contiguous() else t


class GBDTClassifier:
    def __init__(self, n_estimators: int = 100, learning_rate: float = 0.1, max_depth: int = 5,
                 reg_lambda: float = 1.0, min_child_weight: float = 1.0, gamma: float = 0.0, max_bin: int = 256,
                 scale_pos_weight: float = 1.0, base_score: float = 0.5, device: str = "auto",
                 eval_metric=None, early_stopping_rounds: int | None = None, subsample: float = 1.0,
                 colsample_bytree: float = 1.0, colsample_bylevel: float = 1.0, colsample_bynode: float = 1.0,
                 seed: int | None = None, random_state: int | None = None, missing_policy: str = "last_bin",
                 monotone_constraints=None, interaction_constraints=None, reg_alpha: float = 0.0,
                 max_delta_step: float = 0.0, **_ignored):
        # xgboost-only knobs the reference passes (objective, n_jobs) are accepted and ignored: the
        # objective is binary:logistic.  eval_metric and early_stopping_rounds are constructor
        # arguments as in xgboost >= 1.6; they act only when fit() gets an eval_set (the reference's
        # call passes none: nothing is evaluated).  subsample / colsample_by* switch stochastic
        # boosting on (ops/gbdt.fit_binned); ``random_state`` is the seed when ``seed`` is not given,
        # and without sampling neither has any effect: the fit is deterministic.
        # missing_policy="learn": rows may hold NaN and every split learns the side they go to
        # (xgboost's handling of missing values; ops/gbdt.fit_binned); the default "last_bin" bins a
        # NaN with the feature's largest values.
        # monotone_constraints: xgboost's forms -- a sequence of -1 / 0 / +1 per feature, the string
        # "(1,0,-1)" or {feature index: sign} (indices, not names: the estimator takes arrays); the
        # fitted margin then never falls (+1) or never rises (-1) as that feature grows.
        # interaction_constraints: xgboost's forms -- a list of groups of feature indices or the string
        # "[[0, 2], [1, 3, 4]]" (indices, not names); below a path of split features a node may then
        # use the path's own features and every group that contains the whole path
        # (ops/reference_gbdt's module docstring has the rule).
        # reg_alpha / max_delta_step: xgboost's L1 regularisation of the leaf weights and its cap on
        # |weight| (0 = off; the knob xgboost recommends for extremely imbalanced logistic fits), both
        # finite and >= 0 (ops/gbdt.fit_binned has the rules).
        if seed is None:
            seed = 0 if random_state is None else random_state
        self.params = gb.GBDTParams(n_estimators=n_estimators, learning_rate=learning_rate, max_depth=max_depth,
                                    reg_lambda=reg_lambda, min_child_weight=min_child_weight, gamma=gamma,
                                    max_bin=max_bin, scale_pos_weight=scale_pos_weight, base_score=base_score,
                                    subsample=subsample, colsample_bytree=colsample_bytree,
                                    colsample_bylevel=colsample_bylevel, colsample_bynode=colsample_bynode,
                                    seed=int(seed), missing_policy=missing_policy,
                                    monotone_constraints=gb.normalize_monotone(monotone_constraints),
                                    interaction_constraints=gb.normalize_interaction(interaction_constraints),
                                    reg_alpha=reg_alpha, max_delta_step=max_delta_step)
        self.device = device
        self.eval_metric = eval_metric
        self.early_stopping_rounds = early_stopping_rounds
        self.ensemble: gb.TreeEnsemble | None = None
        self._dens = None
        self.feature_names_in_ = None
        self.evals_result_: dict | None = None
        self.best_iteration: int | None = None
        self.best_score: float | None = None

    def _dev(self, X):
        if isinstance(X, torch.Tensor) and self.device == "auto":
            return X.device
        if self.device == "auto":
            return torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
        return torch.device(self.device)

    def get_params(self, deep: bool = True) -> dict:
        return dict(self.params.__dict__)

    def __getstate__(self):  # joblib/pickle: plain values and host arrays only (no device tensors)
        st = dict(self.__dict__)
        st["_dens"] = None
        st.pop("_pexpl", None)
        st.pop("_pdexpl", None)
        st.pop("_piexpl", None)
        st["params"] = dict(self.params.__dict__)
        return st

    def __setstate__(self, st):
        st = dict(st)
        st["params"] = gb.GBDTParams(**{k: v for k, v in st["params"].items() if k in _PARAM_FIELDS})
        # models pickled before evaluation existed carry none of its attributes
        for k in ("eval_metric", "early_stopping_rounds", "evals_result_", "best_iteration", "best_score"):
            st.setdefault(k, None)
        self.__dict__.update(st)

    def fit(self, X, y, sample_weight=None, comm=None, eval_set=None, verbose: bool = False,
            sample_weight_eval_set=None, record_cover: bool = False):
        """``eval_set``: ``[(Xv, yv)]`` (exactly one set, xgboost's list form) evaluated after every
        round with the constructor's ``eval_metric`` (a name or a list of "logloss", "error", "auc",
        "aucpr"; default "logloss"; "aucpr" is sklearn's average precision over tie groups, which
        xgboost's ``aucpr`` interpolates slightly differently); with
        ``early_stopping_rounds`` the last metric stops the fit and the model keeps trees
        [: best_iteration + 1] (xgboost keeps the tail and never predicts with it).  Without
        ``eval_set`` nothing is evaluated.

        ``sample_weight``: one weight per row of X (numpy or torch; finite, >= 0, at least one
        positive), multiplied into the row's gradient pair together with ``scale_pos_weight``
        (ops/gbdt.fit_binned has the definitions and the 14-bit resolution limit).
        ``sample_weight_eval_set``: a list with one array, the eval rows' weights, as in xgboost;
        "logloss" and "error" become weighted means, "auc" / "aucpr" with evaluation weights raise
        NotImplementedError.  ``None`` everywhere is the unweighted call.  Out of scope: the quantile
        cuts stay unweighted, and GBDTPipeline, DeviceGBDTCV and the train entry point take no
        weights (SMOTE's synthetic rows have no defined weight; imblearn drops weights too).

        ``record_cover=True``: after the last round, store xgboost's per-node sum_hess of the training
        rows in the model (``compute_cover(X)``; unweighted, this process's rows) so
        ``predict_contribs`` works without another call.  The default enqueues exactly the launches
        it always did."""
        self._fit(X, y, sample_weight, comm, eval_set, verbose, sample_weight_eval_set)
        if record_cover:
            self.compute_cover(X)
        return self

    def _fit(self, X, y, sample_weight, comm, eval_set, verbose, sample_weight_eval_set):
        dev = self._dev(X)
        Xt = _as_tensor(X, dev)
        yt = (y if isinstance(y, torch.Tensor) else torch.from_numpy(np.asarray(y))).to(dev).to(torch.uint8)

        def weights(w):
            if w is None:
                return None
            w = w if isinstance(w, torch.Tensor) else torch.from_numpy(np.asarray(w))
            return w.reshape(-1).to(dev).to(torch.float32).contiguous()

        if sample_weight_eval_set is not None:
            if eval_set is None:
                raise ValueError("sample_weight_eval_set needs an eval_set")
            if isinstance(sample_weight_eval_set, (list, tuple)):
                if len(sample_weight_eval_set) != 1:
                    raise ValueError("sample_weight_eval_set takes exactly one array (one eval set is supported)")
                sample_weight_eval_set = sample_weight_eval_set[0]
        kw = dict(comm=comm, sample_weight=weights(sample_weight))
        self._dens = None
        self.evals_result_, self.best_iteration, self.best_score = None, None, None
        if eval_set is None:
            if self.early_stopping_rounds is not None:
                raise ValueError("early_stopping_rounds needs fit(..., eval_set=[(Xv, yv)])")
            self.ensemble = gb.fit(Xt, yt.contiguous(), self.params, **kw)
            return self
        if isinstance(eval_set, tuple):
            eval_set = [eval_set]
        if len(eval_set) != 1:
            raise ValueError("exactly one eval set is supported")
        Xv, yv = eval_set[0]
        Xv = _as_tensor(Xv, dev)
        yv = (yv if isinstance(yv, torch.Tensor) else torch.from_numpy(np.asarray(yv))).to(dev).to(torch.uint8)
        metrics = self.eval_metric if self.eval_metric is not None else "logloss"
        self.ensemble, rec = gb.fit(Xt, yt.contiguous(), self.params, eval_set=(Xv, yv.contiguous()),
                                    eval_metric=metrics, early_stopping_rounds=self.early_stopping_rounds,
                                    eval_sample_weight=weights(sample_weight_eval_set), **kw)
        self.evals_result_ = {"validation_0": {k: list(v) for k, v in rec.history.items()}}
        self.best_iteration, self.best_score = rec.best_iteration, rec.best_score
        if verbose:
            for t in range(rec.n_rounds):
                print(f"[{t}]\t" + "\t".join(f"validation_0-{k}:{v[t]:.5f}" for k, v in rec.history.items()))
        return self

    def evals_result(self) -> dict:
        """``{"validation_0": {metric: [value per round]}}`` of the last fit with an eval_set."""
        if self.evals_result_ is None:
            raise RuntimeError("no evaluation was run: pass eval_set to fit()")
        return self.evals_result_

    def _check(self):
        if self.ensemble is None:
            raise RuntimeError("model is not fitted")

    def _n_trees(self, iteration_range):
        """Trees a predict call uses: all of the (kept) ensemble, or the first k of (0, k)."""
        if iteration_range is None:
            return None
        lo, hi = (int(v) for v in iteration_range)
        if lo != 0:
            raise ValueError("iteration_range must start at 0")
        return self.ensemble.n_trees if hi == 0 else hi  # (0, 0) means every tree, as in xgboost

    def predict_margin(self, X, iteration_range=None) -> np.ndarray:
        self._check()
        dev = self._dev(X)
        Xt = _as_tensor(X, dev)
        if Xt.is_cuda and (self._dens is None or self._dens.device != Xt.device):
            self._dens = gb.DeviceEnsemble(self.ensemble, Xt.device)
        return gb.predict_margin(Xt, self.ensemble, self._dens, n_trees=self._n_trees(iteration_range)).cpu().numpy()

    def predict_proba(self, X, iteration_range=None) -> np.ndarray:
        p = 1.0 / (1.0 + np.exp(-self.predict_margin(X, iteration_range).astype(np.float64)))
        return np.stack([1.0 - p, p], 1)

    def predict(self, X, iteration_range=None) -> np.ndarray:
        return (self.predict_margin(X, iteration_range) > 0.0).astype(np.int64)

    def compute_cover(self, X, kind: str = "hessian") -> "GBDTClassifier":
        """Store the node covers of the fitted trees over the rows X in the model (ops/gbdt.node_cover):
        ``kind="hessian"`` is xgboost's sum_hess, ``"count"`` the rows per node.  They are what
        ``predict_contribs`` and the "cover" importances read, and ``save_model`` writes them."""
        self._check()
        dev = self._dev(X)
        Xt = _as_tensor(X, dev)
        if Xt.is_cuda and (self._dens is None or self._dens.device != Xt.device):
            self._dens = gb.DeviceEnsemble(self.ensemble, Xt.device)
        q = gb.node_cover(Xt, self.ensemble, kind, self._dens).cpu().numpy()
        self.ensemble = self.ensemble.with_cover(q, kind)
        if self._dens is not None:
            self._dens.ens = self.ensemble
        self._pexpl = None
        return self

    def predict_contribs(self, X, iteration_range=None) -> np.ndarray:
        """xgboost's ``predict(pred_contribs=True)``: float64 [n, d + 1] path-dependent TreeSHAP values
        of the margin from the stored node covers, the last column the bias f0; every row sums to
        ``predict_margin``.  A NaN follows the learned default direction.  ``iteration_range=(0, k)``
        uses the first k trees and their covers.  Needs ``compute_cover`` (or
        ``fit(..., record_cover=True)``) first."""
        expl, Xh = self._path_explainer(X, iteration_range, "predict_contribs")
        phi, _, f0 = expl.explain(Xh)
        return np.concatenate([phi, np.full((phi.shape[0], 1), f0)], 1)

    def predict_interactions(self, X, iteration_range=None) -> np.ndarray:
        """xgboost's ``predict(pred_interactions=True)``: float64 [n, d + 1, d + 1] SHAP interaction
        values of the margin from the stored node covers.  ``[:, :d, :d]`` holds the interactions
        (symmetric), ``[:, d, d]`` the bias f0 and the rest of the last row and column is 0, so every
        ``[:, i, :]`` sums to column i of ``predict_contribs`` and the whole matrix to
        ``predict_margin``.  Covers, NaN routing and ``iteration_range`` as ``predict_contribs``,
        whose cached explainer it shares."""
        expl, Xh = self._path_explainer(X, iteration_range, "predict_interactions")
        inter, _, _, f0 = expl.explain_interactions(Xh)
        n, d = inter.shape[0], inter.shape[1]
        out = np.zeros((n, d + 1, d + 1))
        out[:, :d, :d] = inter
        out[:, d, d] = f0
        return out

    def _path_explainer(self, X, iteration_range, who: str):
        """(the cached TreePathExplainer of the first k trees on X's device, X as fp32 numpy)."""
        self._check()
        if self.ensemble.cover is None:
            raise ValueError(f"{who} needs node covers: call compute_cover(X) (ops/gbdt.node_cover) or "
                             "fit(..., record_cover=True) first")
        from .explainers import TreePathExplainer

        k = self._n_trees(iteration_range)
        k = self.ensemble.n_trees if k is None else k
        dev = self._dev(X)
        cache = getattr(self, "_pexpl", None)
        key = (k, str(dev), id(self.ensemble))
        if cache is None or cache[0] != key:
            d = self.ensemble.n_features
            cache = (key, TreePathExplainer(self.ensemble.head(k), np.zeros(d), np.ones(d), device=str(dev)))
            self._pexpl = cache
        Xh = X.detach().cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X)
        return cache[1], np.ascontiguousarray(Xh, np.float32)

    def partial_dependence(self, X, features, method: str = "brute", kind: str = "average", iteration_range=None):
        """sklearn.inspection.partial_dependence for this model, on the margin (log-odds) and over the
        COMPLETE grid: one cell per interval between the model's thresholds on the feature (an int, or
        a pair of ints for a 2-D surface), plus a "missing" cell on a ``missing_policy="learn"`` model.
        ``method="brute"`` averages the rows X with the feature placed in each cell (exact integer
        sums, bitwise reproducible); ``"recursion"`` needs the node covers instead of rows (X may be
        None) and differs from brute wherever features interact.  ``kind``: "average", or
        "individual" / "both", which also return the ICE curves (float32 [n, cells], bit for bit
        ``predict_margin`` of the modified rows; the average comes with them either way).  Returns a
        ``models.explainers.PartialDependence``; ``iteration_range=(0, k)`` uses the first k trees."""
        self._check()
        if kind not in ("average", "individual", "both"):
            raise ValueError('kind must be "average", "individual" or "both"')
        from .explainers import TreePartialDependence

        k = self._n_trees(iteration_range)
        k = self.ensemble.n_trees if k is None else k
        dev = self._dev(X) if X is not None else torch.device("cpu")
        cache = getattr(self, "_pdexpl", None)
        key = (k, str(dev), id(self.ensemble))
        if cache is None or cache[0] != key:
            d = self.ensemble.n_features
            cache = (key, TreePartialDependence(self.ensemble.head(k), np.zeros(d), np.ones(d), device=str(dev)))
            self._pdexpl = cache
        if method == "recursion":
            return cache[1].partial_dependence(None, features, "recursion", ice=kind != "average")
        Xh = X.detach().cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X)
        return cache[1].partial_dependence(Xh, features, method, ice=kind != "average")

    def permutation_importance(self, X, y, scoring: str = "auc", n_repeats: int = 5, seed: int = 0, features=None,
                               iteration_range=None):
        """sklearn.inspection.permutation_importance for this model: the drop of the metric on the
        rows (X, y) -- held-out rows, untouched by resampling or reweighting -- when one feature is
        permuted among them, ``n_repeats`` times per feature.  ``scoring``: "auc", "aucpr" (average
        precision) or "logloss" (negative log-loss), higher is better; ``features``: the feature
        indices to permute (None: all); ``seed``: an integer in [0, 2^32).  Margins and scores are
        exact (bit for bit ``predict_margin`` on the permuted rows, integer metric sums), so CPU and
        device agree exactly.  Returns a ``models.explainers.PermutationImportance``;
        ``iteration_range=(0, k)`` uses the first k trees."""
        self._check()
        from .explainers import TreePermutationImportance

        k = self._n_trees(iteration_range)
        k = self.ensemble.n_trees if k is None else k
        dev = self._dev(X)
        cache = getattr(self, "_piexpl", None)
        key = (k, str(dev), id(self.ensemble))
        if cache is None or cache[0] != key:
            d = self.ensemble.n_features
            cache = (key, TreePermutationImportance(self.ensemble.head(k), np.zeros(d), np.ones(d), device=str(dev)))
            self._piexpl = cache
        return cache[1].permutation_importance(X, y, scoring, n_repeats, seed, features)

    def feature_importance(self, kind: str = "gain") -> np.ndarray:
        """``TreeEnsemble.feature_importance``: "gain", "weight", "total_gain", "cover", "total_cover"."""
        self._check()
        return self.ensemble.feature_importance(kind)

    @property
    def feature_importances_(self) -> np.ndarray:
        self._check()
        imp = self.ensemble.feature_importance("gain")
        s = imp.sum()
        return imp / s if s > 0 else imp

    def save_model(self, path: str, feature_names=None):
        self._check()
        o = self.ensemble.to_dict()
        o["feature_names"] = list(feature_names) if feature_names is not None else self.feature_names_in_
        with open(path, "w") as f:
            json.dump(o, f)

    @classmethod
    def load_model(cls, path: str, device: str = "auto") -> "GBDTClassifier":
        with open(path) as f:
            o = json.load(f)
        ens = gb.TreeEnsemble.from_dict(o)
        m = cls(device=device, **{k: v for k, v in ens.params.items() if k in _PARAM_FIELDS})
        m.ensemble = ens
        m.feature_names_in_ = o.get("feature_names")
        return m


@dataclass
class GBDTResult:
    scaler: scaler_ops.ScalerStats
    ensemble: gb.TreeEnsemble
    n_rows: int
    n_train_rows: int
    n_minority: int
    n_synthetic: int
    scale_pos_weight: float
    timings: dict = field(default_factory=dict)
    _dens: object = None

    def standardize(self, X: torch.Tensor) -> torch.Tensor:
        rows = scaler_ops.scale_cast(X, self.scaler, out_dtype="f32")
        return rows[:, : self.scaler.d]

    def predict_margin(self, X: torch.Tensor) -> torch.Tensor:
        Xs = self.standardize(X)
        if Xs.is_cuda and (self._dens is None or self._dens.device != Xs.device):
            self._dens = gb.DeviceEnsemble(self.ensemble, Xs.device)
        return gb.predict_margin(Xs, self.ensemble, self._dens)

    def evaluate(self, X: torch.Tensor, y: torch.Tensor, comm=None) -> dict:
        margin = self.predict_margin(X)
        if comm is not None and comm.world_size > 1:
            margin, _ = comm.all_gather_rows(margin.reshape(-1, 1))
            y, _ = comm.all_gather_rows(y.reshape(-1, 1))
            margin, y = margin.reshape(-1).contiguous(), y.reshape(-1).contiguous()
        auc = metric_ops.roc_auc(margin, y)
        tn, fp, fn, tp = (int(v) for v in metric_ops.confusion_counts(margin, y, 0.0))
        return {"auc": auc, "average_precision": metric_ops.average_precision(margin, y),
                "tn": tn, "fp": fp, "fn": fn, "tp": tp, "recall": tp / max(tp + fn, 1),
                "precision": tp / max(tp + fp, 1), "accuracy": (tp + tn) / max(tn + fp + fn + tp, 1)}

    def save(self, model_dir: str, feature_names) -> dict:
        from ..compat.sklearn_export import MARKER, make_scaler
        import joblib

        os.makedirs(model_dir, exist_ok=True)
        mean, var, scale = self.scaler.numpy()
        paths = {"model": os.path.join(model_dir, MODEL_FILE), "joblib": os.path.join(model_dir, JOBLIB_FILE),
                 "scaler": os.path.join(model_dir, "scaler.joblib"),
                 "columns": os.path.join(model_dir, "columns.joblib"),
                 "feature_names": os.path.join(model_dir, "feature_names.json")}
        o = self.ensemble.to_dict()
        o["feature_names"] = list(feature_names)
        o["scale_pos_weight"] = self.scale_pos_weight
        with open(paths["model"], "w") as f:
            json.dump(o, f)
        clf = GBDTClassifier(**{k: v for k, v in self.ensemble.params.items() if k in _PARAM_FIELDS})
        clf.params.scale_pos_weight = float(self.scale_pos_weight)
        clf.ensemble, clf.feature_names_in_ = self.ensemble, list(feature_names)
        joblib.dump(clf, paths["joblib"])
        joblib.dump(make_scaler(mean, var, scale, int(self.scaler.n), feature_names), paths["scaler"])
        joblib.dump(list(feature_names), paths["columns"])
        with open(paths["feature_names"], "w") as f:
            json.dump(list(feature_names), f)
        prov = os.path.join(model_dir, ".fdx_provenance.json")
        meta = {}
        if os.path.exists(prov):
            with open(prov) as f:
                meta = json.load(f)
        meta.update(writer=MARKER, gbdt_model=MODEL_FILE, gbdt_joblib=JOBLIB_FILE)
        meta.setdefault("model", meta.get("model", "logistic_model.joblib"))
        with open(prov, "w") as f:
            json.dump(meta, f)
        return paths

    def log_model(self, mlf, paths: dict) -> str:
        files = {MODEL_FILE: paths["model"], "scaler.joblib": paths["scaler"],
                 "feature_names.json": paths["feature_names"]}
        if paths.get("background"):
            files["shap_background.npy"] = paths["background"]
        return mlf.log_files_model(files, "model", "fdx_gbdt",
                                   {"model_file": MODEL_FILE, "format": "fdx-gbdt/1", "depth": self.ensemble.depth,
                                    "n_trees": self.ensemble.n_trees})


class GBDTPipeline:
    def __init__(self, cfg: TrainConfig | None = None, params: gb.GBDTParams | None = None, comm=None,
                 scale_pos_weight: float | str = "auto", checkpoint_dir: str | None = None,
                 checkpoint_every: int = 10):
        self.cfg = cfg or TrainConfig()
        self.params = params or gb.GBDTParams()
        if self.params.learn_missing:
            raise NotImplementedError('GBDTPipeline does not support missing_policy="learn": the scaler, k-NN and '
                                      "SMOTE of the recipe have no NaN semantics; use GBDTClassifier")
        self.comm = comm
        self.spw = scale_pos_weight
        self.checkpoint_dir, self.checkpoint_every = checkpoint_dir, checkpoint_every

    def fit(self, X: torch.Tensor, y: torch.Tensor) -> GBDTResult:
        cfg = self.cfg
        comm = self.comm if (self.comm is not None and self.comm.world_size > 1) else None
        rank = comm.rank if comm else 0
        t = {}
        t0 = time.perf_counter()
        n, d = X.shape
        stats = scaler_ops.scaler_fit(X, comm=comm)
        idx_min = scaler_ops.compact_indices(y, 1)
        n_min = int(idx_min.shape[0])
        def quota(n_r, nmin_r):
            return max(0, int(round((n_r - nmin_r) * cfg.sampling_ratio)) - nmin_r) if (cfg.smote and nmin_r > 0) else 0

        # SMOTE: single process, or under DP the exact global scheme of models/pipeline.py (every
        # rank a 128-aligned slice of one global draw sequence over all minority rows)
        ranks = comm.all_gather_ints([n_min, n]) if comm else [[n_min, n]]
        if comm:
            per, s_off = global_smote_slices(ranks, quota, rank)
        else:
            per, s_off = [quota(n, n_min)], 0
        n_new = per[rank]
        neg = float(sum(r[1] - r[0] for r in ranks))
        pos = float(sum(r[0] for r in ranks))
        if self.spw == "auto":  # the fitted rows' balance (post-SMOTE)
            spw = neg / (pos + sum(per)) if pos + sum(per) > 0 else 1.0
        elif self.spw == "reference":  # train_model.py:52-54 (pre-SMOTE, App. D #11)
            spw = neg / pos if pos > 0 else 1.0
        else:
            spw = float(self.spw)
        rows = torch.empty((n + n_new, NCOLS), dtype=torch.float32, device=X.device)
        scaler_ops.scale_cast(X, stats, labels=y, out_dtype="f32", out=rows[:n])
        if sum(per) > 0:
            xmin = rows[:n].index_select(0, idx_min).contiguous()
            counts = [r[0] for r in ranks]
            xall = comm.all_gather_rows(xmin, counts=counts)[0] if comm else xmin
            q_off = int(sum(counts[:rank]))
            k = min(cfg.k_neighbors, xall.shape[0] - 1)
            if k < 1:
                raise ValueError("SMOTE needs at least 2 minority samples")
            nbr = knn_ops.knn_topk(xmin, xall, k=k, self_offset=q_off) if n_min > 0 else \
                torch.empty((0, k), dtype=torch.int32, device=X.device)
            if comm:
                nbr = comm.all_gather_rows(nbr, counts=counts)[0]
            if n_new > 0:
                knn_ops.smote_generate(xall, nbr, 0, n_new, rows[n:], seed=cfg.seed, counter_base=0,
                                       sample_offset=s_off)
        labels = torch.empty(n + n_new, dtype=torch.uint8, device=X.device)
        labels[:n] = y
        labels[n:] = 1
        t["prep"] = time.perf_counter() - t0
        params = gb.GBDTParams(**{**self.params.__dict__, "scale_pos_weight": spw})
        ck = None
        if self.checkpoint_dir:
            from ..utils.checkpoint import CheckpointManager

            ck = CheckpointManager(self.checkpoint_dir, prefix="gbdt", keep=2, rank=rank)
        ens = gb.fit(rows[:, :d], labels, params, comm=comm, checkpoint=ck, checkpoint_every=self.checkpoint_every)
        t["boost"] = time.perf_counter() - t0 - t["prep"]
        return GBDTResult(scaler=stats, ensemble=ens, n_rows=n, n_train_rows=n + n_new, n_minority=n_min,
                          n_synthetic=n_new, scale_pos_weight=spw, timings=t)
