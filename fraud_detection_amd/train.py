"""Training entry point behind train_model.py (reference call stack: SURVEY.md §3.1).

    read CSV (native reader) -> stratified 80/20 split (rs=42)
    -> StratifiedKFold(5, shuffle, rs=42): per fold the device pipeline (scaler on the fold's
       train rows -> SMOTE k-NN + generation -> fit) and the fold's validation AUC
    -> final pipeline on the whole train split -> exact test AUC
    -> artifacts in the reference layout (models/logistic_model.joblib, scaler.joblib,
       columns.joblib, feature_names.json; for the GBDT family models/xgb_model.joblib -- a
       GBDTClassifier, the reference's joblib contract -- plus models/xgb_model.json, the
       pickle-free copy serving loads)
    -> MLflow run (params model_type / scale_pos_weight / cv_folds, metrics test_auc /
       cv_auc_mean / cv_auc_std, sklearn model with signature + input example, scaler artifact),
       registration when test_auc >= MLFLOW_AUC_THRESHOLD and the serving alias set to
       MLFLOW_MODEL_STAGE.  Tracking failures never fail training (train_model.py:165-166).
"""
from __future__ import annotations

import json
import logging
import os
import tempfile
import time

import numpy as np
import torch

from .compat import mlflow_compat as mlf
from .compat.sklearn_export import LinearArtifacts, make_logistic, save_artifacts
from .config import Settings
from .data.io import missing_report, read_table, stratified_folds, stratified_split
from .models.pipeline import DevicePipeline, TrainConfig, evaluate
from .obs import tracing
from .obs.metrics import train_metrics
from .runtime.hbm import observe_hbm

logger = logging.getLogger("train")

DEVICE_SPLIT_ROWS = 2_000_000
FOLD_PARALLEL_ROWS = 8_000_000


def _device(name: str) -> torch.device:
    if name == "auto":
        return torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    return torch.device(name)


def _shard(idx: np.ndarray, comm) -> np.ndarray:
    """This rank's rows of an index set (strided, so every shard keeps the class mix)."""
    if comm is None:
        return idx
    return idx[comm.rank::comm.world_size]


def parse_gbdt_monotone(spec: str | None, names) -> dict | None:
    """``--gbdt-monotone "Amount=1,V14=-1"`` -> {feature index: sign}, the names resolved against the
    table's feature columns.  None / empty: no constraints.  An unknown or repeated name, or a sign
    other than -1, 0, 1, is a ValueError."""
    if spec is None or not spec.strip():
        return None
    names = list(names)
    out = {}
    for item in spec.split(","):
        name, eq, val = item.partition("=")
        name, val = name.strip(), val.strip()
        if not eq or not name:
            raise ValueError(f"--gbdt-monotone: expected NAME=SIGN, got {item.strip()!r}")
        if name not in names:
            raise ValueError(f"--gbdt-monotone: the table has no feature column {name!r}")
        if val not in ("-1", "0", "1", "+1"):
            raise ValueError(f"--gbdt-monotone: the sign of {name!r} must be -1, 0 or 1, got {val!r}")
        if names.index(name) in out:
            raise ValueError(f"--gbdt-monotone: {name!r} is named twice")
        out[names.index(name)] = int(val)
    return out


def parse_gbdt_interaction(spec: str | None, names) -> list | None:
    """``--gbdt-interaction "Amount,Time;V14,V17,V12"`` -> [[feature index, ...], ...]: groups
    separated by ``;``, column names by ``,``, the names resolved against the table's feature
    columns.  None / empty: no constraints.  An unknown name, a name repeated inside one group or an
    empty group is a ValueError."""
    if spec is None or not spec.strip():
        return None
    names = list(names)
    out = []
    for group in spec.split(";"):
        idx = []
        for name in group.split(","):
            name = name.strip()
            if not name:
                raise ValueError(f"--gbdt-interaction: expected NAME,NAME;NAME,..., got {group.strip()!r}")
            if name not in names:
                raise ValueError(f"--gbdt-interaction: the table has no feature column {name!r}")
            if names.index(name) in idx:
                raise ValueError(f"--gbdt-interaction: {name!r} is named twice in one group")
            idx.append(names.index(name))
        out.append(idx)
    return out


def run(settings: Settings | None = None, model_type: str = "logistic", cv_folds: int = 5, model_dir: str = "models",
        verbose: bool = True, cfg: TrainConfig | None = None, comm=None, gbdt_eval_metric=None,
        gbdt_early_stopping: int | None = None, gbdt_subsample: float = 1.0, gbdt_colsample_bytree: float = 1.0,
        gbdt_seed: int = 0, gbdt_monotone: str | None = None, gbdt_interaction: str | None = None,
        gbdt_reg_alpha: float = 0.0, gbdt_max_delta_step: float = 0.0, gbdt_cover: str | None = None) -> dict:
    """Single process, or data parallel when ``comm`` spans several ranks (torchrun: one rank per
    GPU).  Every rank reads the table and derives the same split; each fits on its strided shard
    with RCCL all-reduced statistics, so all ranks hold the same model; rank 0 writes artifacts.

    ``gbdt_eval_metric`` / ``gbdt_early_stopping``: per-round validation metrics of every CV fold
    and early stopping in the device GBDT CV job (models/gbdt_cv.DeviceGBDTCV); the curves, best
    rounds and the final fit's round count land in the summary under "gbdt_eval".

    ``gbdt_subsample`` / ``gbdt_colsample_bytree`` / ``gbdt_seed``: stochastic boosting of the GBDT
    family (ops/gbdt.GBDTParams), in every CV fold and in the final fit alike.

    ``gbdt_monotone``: "Amount=1,V14=-1" -- monotone constraints by column name (parse_gbdt_monotone),
    in every CV fold and in the final fit; standardisation divides by a positive scale, so a sign on
    the raw column is the same sign on the standardised one.  The chosen signs land in the summary
    under "gbdt_monotone".

    ``gbdt_interaction``: "Amount,Time;V14,V17,V12" -- interaction constraints by column name
    (parse_gbdt_interaction), in every CV fold and in the final fit.  The groups land in the summary
    under "gbdt_interaction", by name.

    ``gbdt_reg_alpha`` / ``gbdt_max_delta_step``: xgboost's L1 regularisation of the leaf weights and
    its cap on |weight| (ops/gbdt.GBDTParams; both finite and >= 0, 0 = off), in every CV fold and in
    the final fit.  Non-zero values land in the summary under "gbdt_reg".

    ``gbdt_cover``: "hessian" or "count" -- after the final fit, node covers (ops/gbdt.node_cover) over
    the REAL standardized training rows are stored in xgb_model.json, so the deployed engine serves
    path-dependent TreeSHAP (``tree_path``) with no background file.  xgboost's sum_hess is taken
    over the rows the trees were fit on, which here would include SMOTE's synthetic rows: the
    covers deliberately describe the real data distribution instead.  Without it the saved model
    is byte for byte what it always was."""
    s = settings or Settings.load()
    comm = comm if (comm is not None and comm.world_size > 1) else None
    lead = comm is None or comm.rank == 0
    say = print if (verbose and lead) else (lambda *a, **k: None)
    dev = _device(s.device)
    if comm is not None and dev.type == "cuda":
        dev = torch.device("cuda", torch.cuda.current_device())
    t0 = time.time()
    say("Loading dataset...")
    X, y, names = read_table(s.data_csv)
    if y is None:
        raise ValueError(f"{s.data_csv} has no 'Class' column")
    say("Checking missing values...")
    miss = missing_report(X, names)
    say({k: v for k, v in miss.items() if v} or "no missing values")
    if any(miss.values()):
        raise ValueError("missing feature values; impute before training (this entry point's scaler and SMOTE "
                         'have no NaN semantics; GBDTClassifier(missing_policy="learn") learns from them)')
    say("Splitting dataset (Train 80% / Test 20%)...")
    mode = s.split
    if mode == "auto":  # the sklearn split is a host argsort: past a few million rows use K3
        mode = "device" if dev.type == "cuda" and X.shape[0] >= DEVICE_SPLIT_ROWS else "sklearn"
    if mode == "device":
        from .ops import split as SP

        Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)  # one upload, then on-device gathers
        codes = SP.assign(yd, 0.2, cv_folds if cv_folds and cv_folds > 1 else 0, 42)
        tr, te, dev_folds = SP.split_indices(codes, cv_folds if cv_folds and cv_folds > 1 else 0)
        take = lambda idx: (Xd.index_select(0, idx), yd.index_select(0, idx))  # noqa: E731
        pos = int(yd.index_select(0, tr).sum())
        neg = int(tr.shape[0]) - pos
    elif mode == "sklearn":
        tr, te = stratified_split(y, 0.2, 42)
        take = lambda idx: (torch.from_numpy(X[idx]).to(dev), torch.from_numpy(y[idx]).to(dev))  # noqa: E731
        neg, pos = int((y[tr] == 0).sum()), int((y[tr] == 1).sum())
    else:
        raise ValueError("split must be sklearn | device | auto")
    Xtr, ytr = take(_shard(tr, comm))
    Xte, yte = take(_shard(te, comm))
    scale_pos_weight = neg / pos if pos > 0 else 1.0
    say(f" Class balance before SMOTE -> [{neg} {pos}]")
    cfg = cfg or TrainConfig(solver=s.solver, storage=s.dtype, seed=s.seed, k_neighbors=s.smote_k)
    if model_type not in ("logistic", "gbdt"):
        raise ValueError("model_type must be 'logistic' or 'gbdt'")
    gbdt_params = None
    if model_type == "gbdt":
        from .ops.gbdt import GBDTParams

        gbdt_mono = parse_gbdt_monotone(gbdt_monotone, names)
        gbdt_params = GBDTParams(subsample=gbdt_subsample, colsample_bytree=gbdt_colsample_bytree,
                                 seed=gbdt_seed, monotone_constraints=gbdt_mono,
                                 interaction_constraints=parse_gbdt_interaction(gbdt_interaction, names),
                                 reg_alpha=gbdt_reg_alpha, max_delta_step=gbdt_max_delta_step).validate()
    elif (gbdt_subsample, gbdt_colsample_bytree, gbdt_seed) != (1.0, 1.0, 0):
        raise ValueError("--gbdt-subsample / --gbdt-colsample-bytree / --gbdt-seed need --model gbdt")
    elif gbdt_monotone:
        raise ValueError("--gbdt-monotone needs --model gbdt")
    elif gbdt_interaction:
        raise ValueError("--gbdt-interaction needs --model gbdt")
    elif gbdt_reg_alpha or gbdt_max_delta_step:
        raise ValueError("--gbdt-reg-alpha / --gbdt-max-delta-step need --model gbdt")
    if gbdt_cover is not None:
        if model_type != "gbdt":
            raise ValueError("--gbdt-cover needs --model gbdt")
        if gbdt_cover not in ("hessian", "count"):
            raise ValueError("--gbdt-cover must be hessian or count")
        if comm is not None and comm.world_size > 1:  # the int64 tables would add across ranks: not wired up
            raise ValueError("--gbdt-cover runs in a single process (data-parallel covers are not implemented)")
    cv_scores = []
    from dataclasses import asdict

    ck_dir = s.checkpoint_dir or None
    progress = _Progress(ck_dir, lead, signature=None if ck_dir is None else _job_signature(
        s, model_type, cv_folds, mode, asdict(cfg), X.shape, comm, gbdt_params))
    if progress.folds:
        say(f" Resuming: {len(progress.folds)} completed fold(s) from {progress.path}")
    res_cv = None
    cv_engine = None
    gbdt_eval = None
    if (gbdt_eval_metric is not None or gbdt_early_stopping is not None) and not (
            cv_folds and cv_folds > 1 and pos >= cv_folds and _device_gbdt_cv_ok(model_type, cfg, dev, comm, progress)):
        raise ValueError("--gbdt-eval-metric / --gbdt-early-stopping need the device GBDT CV job "
                         "(--model gbdt on one GPU with CV folds, not resumed)")
    if cv_folds and cv_folds > 1 and pos >= cv_folds:
        say(f" Performing Stratified K-Fold Cross-Validation ({cv_folds} folds) with SMOTE inside each fold...")
        if mode == "device":
            folds = dev_folds
            # the device jobs run on the K3 codes of this split (the per-fold path's folds)
            job_codes = codes.index_select(0, tr) if comm is None else None
        else:
            sk = stratified_folds(y[tr], cv_folds, 42)
            folds = [(tr[a], tr[b]) for a, b in sk]
            # sklearn's StratifiedKFold(5, shuffle, 42) membership (train_model.py:49,58) for the
            # device jobs too: their fold AUCs are on the reference's folds
            job_codes = None
            if comm is None:
                from .models.cv import fold_codes_from_splits

                job_codes = fold_codes_from_splits(sk, len(tr))
        cv_mode = s.cv_parallel
        if cv_mode == "auto":  # small folds are latency-bound under DP: give each rank whole folds
            cv_mode = "fold" if comm is not None and len(tr) < FOLD_PARALLEL_ROWS else "dp"
        if _device_cv_ok(model_type, cfg, dev, comm, progress, Xtr):
            # models/cv.DeviceCV: the reference's semantics (ONE scaler on the training split,
            # SMOTE inside every fold) on one fold-sorted device table, final fit included
            from .models.cv import DeviceCV

            t_fit = time.perf_counter()
            with tracing.span("train.cv_job", model=model_type), tracing.roctx_range("train.cv_job"):
                cvr = DeviceCV(cfg, cv_folds, seed=42).run(Xtr, ytr, fold_codes=job_codes)
            cv_scores, res_cv, cv_engine = cvr.fold_aucs, cvr.final, "device"
            for k, auc in enumerate(cv_scores):
                progress.record(k, auc)
        elif _device_gbdt_cv_ok(model_type, cfg, dev, comm, progress):
            # models/gbdt_cv.DeviceGBDTCV: one binned fold-sorted table, fold k fits around its own
            # block (row hole, no copy), its margins are the validation scores; final fit included
            from .models.gbdt_cv import DeviceGBDTCV

            t_fit = time.perf_counter()
            with tracing.span("train.cv_job", model=model_type), tracing.roctx_range("train.cv_job"):
                cvr = DeviceGBDTCV(cfg, params=gbdt_params, n_folds=cv_folds, seed=42, eval_metric=gbdt_eval_metric,
                                   early_stopping_rounds=gbdt_early_stopping).run(Xtr, ytr, fold_codes=job_codes)
            cv_scores, res_cv, cv_engine = cvr.fold_aucs, cvr.final, "device"
            if cvr.fold_evals:
                gbdt_eval = {"metrics": list(cvr.fold_evals[0].metrics), "early_stopping_rounds": gbdt_early_stopping,
                             "fold_history": [r.history for r in cvr.fold_evals],
                             "fold_best_iteration": list(cvr.fold_best_iteration),
                             "fold_best_score": [r.best_score for r in cvr.fold_evals],
                             "final_n_estimators": cvr.final_n_estimators}
            for k, auc in enumerate(cv_scores):
                progress.record(k, auc)
        else:
            cv_scores = _cross_validate(model_type, cfg, folds, take, comm, cv_mode, progress, gbdt_params)
            cv_engine = f"per_fold:{cv_mode}"
        for k, auc in enumerate(cv_scores):
            say(f"  Fold {k + 1} AUC: {auc:.4f}")
        say(f" CV AUC Mean: {np.mean(cv_scores):.4f} (+/- {np.std(cv_scores) * 2:.4f})")
    say(f" Training final {model_type} model with SMOTE on the full training set...")
    if res_cv is None:
        t_fit = time.perf_counter()
        with tracing.span("train.final_fit", model=model_type), tracing.roctx_range("train.final_fit"):
            res = _fit(model_type, cfg, Xtr, ytr, comm,
                       checkpoint=None if ck_dir is None else os.path.join(ck_dir, f"final_{model_type}"),
                       gbdt_params=gbdt_params)
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
    else:
        res = res_cv  # fitted inside the CV job (t_fit: the whole job)
    t_fit = time.perf_counter() - t_fit
    tm = train_metrics()
    tm.rows_per_second.set(float(res.n_train_rows) * (comm.world_size if comm else 1) / max(t_fit, 1e-9))
    observe_hbm(dev)
    if model_type == "gbdt":  # the weight the trees were fit with (post-SMOTE balance by default)
        scale_pos_weight = float(res.scale_pos_weight)
    if model_type == "logistic":
        ev = evaluate(res, Xte, yte, comm)
        auc = ev["auc"]
        say(f" Class balance after SMOTE -> [{res.n_rows - res.n_minority} {res.n_minority + res.n_synthetic}]"
            + (f" (rank 0 of {comm.world_size})" if comm else ""))
    else:
        ev = res.evaluate(Xte, yte, comm)
        auc = ev["auc"]
    say(f"Test AUC: {auc:.4f}")
    if not lead:
        comm.barrier()
        return {"test_auc": float(auc), "cv_scores": cv_scores, "rank": comm.rank}
    if gbdt_cover is not None:
        from .ops import gbdt as gb_ops

        res.ensemble = res.ensemble.with_cover(
            gb_ops.node_cover(res.standardize(Xtr), res.ensemble, gbdt_cover).cpu().numpy(), gbdt_cover)
        res._dens = None
    paths = _save(model_type, res, names, model_dir, cfg)
    # KernelSHAP background (shap.sample of the training rows) for the async XAI worker
    from .serve.engine import sample_background, save_background

    paths["background"] = save_background(sample_background(Xtr[: 1 << 20].cpu().numpy(), s.kernelshap_background,
                                                            s.seed), model_dir)
    say(f" Model and scaler saved to /{model_dir}")
    summary = {"test_auc": float(auc), "cv_auc_mean": float(np.mean(cv_scores)) if cv_scores else None,
               "cv_auc_std": float(np.std(cv_scores)) if cv_scores else None, "cv_scores": cv_scores,
               "scale_pos_weight": scale_pos_weight, "paths": paths, "device": str(dev), "eval": ev,
               "seconds": round(time.time() - t0, 3), "registered_version": None}
    if gbdt_eval is not None:
        summary["gbdt_eval"] = gbdt_eval
    if gbdt_params is not None and gbdt_params.sampled:
        summary["gbdt_sampling"] = {"subsample": gbdt_params.subsample,
                                    "colsample_bytree": gbdt_params.colsample_bytree, "seed": gbdt_params.seed}
    if gbdt_params is not None and gbdt_params.monotone_constraints:
        summary["gbdt_monotone"] = {names[f]: c for f, c in sorted(gbdt_params.monotone_constraints.items()) if c}
    if gbdt_params is not None and gbdt_params.interaction_constraints:
        summary["gbdt_interaction"] = [[names[f] for f in g] for g in gbdt_params.interaction_constraints]
    if gbdt_cover is not None:
        summary["gbdt_cover"] = {"kind": gbdt_cover, "rows": int(Xtr.shape[0])}
    if gbdt_params is not None and gbdt_params.reg is not None:
        summary["gbdt_reg"] = {"reg_alpha": gbdt_params.reg[0], "max_delta_step": gbdt_params.reg[1]}
    try:
        summary["registered_version"] = _track(s, model_type, res, summary, paths, Xte, names, say)
    except Exception as e:  # noqa: BLE001 - tracking is best effort (reference train_model.py:165-166)
        say(f" MLflow Tracking Failed (likely connection error): {e}")
    summary["split"] = mode
    summary["cv_engine"] = cv_engine
    summary["resumed_folds"] = sorted(progress.resumed)
    if comm is not None:
        summary["world_size"] = comm.world_size
        comm.barrier()
    return summary


class _Progress:
    """Job-level resume: completed CV folds are recorded in
    ``<checkpoint_dir>/train_progress.json`` (atomic rename, rank 0 writes), so a job restarted
    after a crash or a lost rank (``torchrun --max-restarts``) skips them; the final GBDT fit
    resumes from its tree checkpoints.  A record is used only if the job signature (data file,
    model, folds, split, training config, world size) matches."""

    def __init__(self, directory, lead: bool, signature):
        self.path = os.path.join(directory, "train_progress.json") if directory else None
        self.lead, self.sig = lead, signature
        self.folds: dict = {}
        if self.path and os.path.exists(self.path):
            with open(self.path) as f:
                d = json.load(f)
            if d.get("signature") == signature:
                self.folds = {int(k): float(v) for k, v in d.get("folds", {}).items()}
        self.resumed = set(self.folds)

    def record(self, k: int, auc: float):
        self.folds[k] = float(auc)
        if self.path and self.lead:
            os.makedirs(os.path.dirname(self.path), exist_ok=True)
            tmp = self.path + ".tmp"
            with open(tmp, "w") as f:
                json.dump({"signature": self.sig, "folds": self.folds}, f)
            os.replace(tmp, self.path)
        fault = os.getenv("FDX_FAULT", "")
        if fault.startswith("train_crash_after_fold=") and len(self.folds) == int(fault.split("=", 1)[1]):
            logger.error("FDX_FAULT: simulated crash after %d fold(s)", len(self.folds))
            os._exit(17)  # hard exit, like a killed rank: no cleanup, no flush


def _job_signature(s, model_type, cv_folds, split_mode, cfg: dict, shape, comm, gbdt_params=None) -> str:
    from .utils.checkpoint import config_signature

    st = os.stat(s.data_csv)
    return config_signature(data=os.path.abspath(s.data_csv), size=st.st_size, mtime=int(st.st_mtime),
                            shape=list(shape), model=model_type, folds=cv_folds, split=split_mode, cfg=cfg,
                            world=1 if comm is None else comm.world_size,
                            # only when sampling is on: records written before it existed still match
                            **({"gbdt_sampling": [gbdt_params.subsample, gbdt_params.colsample_bytree, gbdt_params.seed]}
                               if gbdt_params is not None and gbdt_params.sampled else {}),
                            **({"gbdt_monotone": sorted(gbdt_params.monotone_constraints.items())}
                               if gbdt_params is not None and gbdt_params.monotone_constraints else {}),
                            **({"gbdt_interaction": [list(g) for g in gbdt_params.interaction_constraints]}
                               if gbdt_params is not None and gbdt_params.interaction_constraints else {}),
                            **({"gbdt_reg": list(gbdt_params.reg)}
                               if gbdt_params is not None and gbdt_params.reg is not None else {}))


def _cross_validate(model_type, cfg, folds, take, comm, mode: str, progress: _Progress | None = None,
                    gbdt_params=None) -> list:
    """K12 per-fold orchestration (train_model.py:58-85).  The table is resident (device split:
    on the GPU), so each fold is an on-device gather, never a host copy.
      dp   -- every fold is fitted data-parallel over all ranks (large folds);
      fold -- fold k runs whole on rank k % world (no collectives inside a fit), and the fold AUCs
              are exchanged once at the end: the fold-parallel mode of SURVEY.md §2.4.
    Folds already in ``progress`` (a resumed job) are not recomputed."""
    progress = progress or _Progress(None, True, None)
    if comm is None or mode == "dp":
        for k, (ftr, fva) in enumerate(folds):
            if k in progress.folds:
                continue
            res = _fit(model_type, cfg, *take(_shard(ftr, comm)), comm, gbdt_params=gbdt_params)
            progress.record(k, _score(model_type, res, *take(_shard(fva, comm)), comm))
        return [progress.folds[k] for k in range(len(folds))]
    if mode != "fold":
        raise ValueError("cv_parallel must be dp | fold | auto")
    mine = {}
    for k in range(comm.rank, len(folds), comm.world_size):
        if k in progress.folds:
            continue
        ftr, fva = folds[k]
        res = _fit(model_type, cfg, *take(ftr), None, gbdt_params=gbdt_params)
        mine[k] = _score(model_type, res, *take(fva), None)
    for part in comm.all_gather_object(mine):
        for k, auc in sorted(part.items()):
            progress.record(k, auc)
    return [progress.folds[k] for k in range(len(folds))]


def _device_cv_ok(model_type, cfg, dev, comm, progress, Xtr) -> bool:
    """The device CV job (models/cv.py) runs the logistic family on one GPU, from scratch (a
    resumed job keeps the per-fold path), with virtual SMOTE (bf16 Newton or SGD in either row
    format) and an even feature count (its gathered scaler pass reads 8-byte row pieces)."""
    if os.environ.get("FDX_CV_ENGINE", "auto") == "per_fold":
        return False
    virt = cfg.solver == "sgd" or (cfg.solver == "newton" and cfg.storage == "bf16")
    return (model_type == "logistic" and dev.type == "cuda" and comm is None and not progress.folds
            and cfg.smote and cfg.virtual_smote and cfg.fold_scaler and virt and Xtr.shape[1] % 2 == 0
            and Xtr.is_contiguous())


def _device_gbdt_cv_ok(model_type, cfg, dev, comm, progress) -> bool:
    """The device GBDT CV job (models/gbdt_cv.py) runs on one GPU, from scratch (a resumed job
    keeps the per-fold path), with SMOTE inside the folds (the reference's semantics)."""
    if os.environ.get("FDX_CV_ENGINE", "auto") == "per_fold":
        return False
    return model_type == "gbdt" and dev.type == "cuda" and comm is None and not progress.folds and cfg.smote


def _fit(model_type, cfg, X, y, comm=None, checkpoint: str | None = None, gbdt_params=None):
    if model_type == "logistic":
        return DevicePipeline(cfg, comm).fit(X, y)
    from .models.gbdt import GBDTPipeline

    return GBDTPipeline(cfg, params=gbdt_params, comm=comm, checkpoint_dir=checkpoint).fit(X, y)


def _score(model_type, res, X, y, comm=None) -> float:
    if model_type == "logistic":
        return float(evaluate(res, X, y, comm)["auc"])
    return float(res.evaluate(X, y, comm)["auc"])


def _save(model_type, res, names, model_dir, cfg) -> dict:
    mean, var, scale = res.scaler.numpy()
    if model_type == "logistic":
        art = LinearArtifacts(coef=res.coef, intercept=res.intercept, mean=mean, var=var, scale=scale,
                              n_samples_seen=int(res.scaler.n), feature_names=names, n_iter=res.fit.n_iter, C=cfg.C)
        return save_artifacts(art, model_dir)
    return res.save(model_dir, names)


def _track(s: Settings, model_type, res, summary, paths, Xte, names, say):
    mlf.set_tracking_uri(s.mlflow_tracking_uri)
    mlf.set_experiment(s.mlflow_experiment)
    version = None
    with mlf.start_run() as run:
        mlf.log_param("model_type", "LogisticRegression" if model_type == "logistic" else "GBDT")
        mlf.log_param("scale_pos_weight", summary["scale_pos_weight"])
        mlf.log_param("cv_folds", len(summary["cv_scores"]) or 0)
        mlf.log_param("device", summary["device"])
        mlf.log_metric("test_auc", summary["test_auc"])
        if summary["cv_auc_mean"] is not None:
            mlf.log_metric("cv_auc_mean", summary["cv_auc_mean"])
            mlf.log_metric("cv_auc_std", summary["cv_auc_std"])
        for k, v in (summary.get("gbdt_sampling") or {}).items():
            mlf.log_param(f"gbdt_{k}", v)
        if summary.get("gbdt_monotone"):
            mlf.log_param("gbdt_monotone", ",".join(f"{k}={v}" for k, v in summary["gbdt_monotone"].items()))
        if summary.get("gbdt_interaction"):
            mlf.log_param("gbdt_interaction", ";".join(",".join(g) for g in summary["gbdt_interaction"]))
        for k, v in (summary.get("gbdt_reg") or {}).items():
            mlf.log_param(f"gbdt_{k}", v)
        ge = summary.get("gbdt_eval")
        if ge:
            mlf.log_param("gbdt_eval_metric", ",".join(ge["metrics"]))
            mlf.log_param("gbdt_early_stopping_rounds", ge["early_stopping_rounds"])
            mlf.log_param("gbdt_final_n_estimators", ge["final_n_estimators"])
            for k, (best, score) in enumerate(zip(ge["fold_best_iteration"], ge["fold_best_score"])):
                mlf.log_metric(f"fold{k + 1}_best_iteration", float(best))
                mlf.log_metric(f"fold{k + 1}_best_{ge['metrics'][-1]}", float(score))
        sample = Xte[:5].cpu().numpy().astype(np.float64)
        if model_type == "logistic":
            model = make_logistic(res.coef, res.intercept, res.fit.n_iter)
            sc = (sample - res.scaler.numpy()[0]) / res.scaler.numpy()[2]
            sig = mlf.infer_signature(sc, model.predict_proba(sc)[:, 1])
            extra = {"scaler.joblib": paths["scaler"], "feature_names.json": paths["feature_names"]}
            if paths.get("background"):
                extra["shap_background.npy"] = paths["background"]
            uri = mlf.log_sklearn_model(model, "model", signature=sig, input_example=sc[:1], extra_files=extra)
        else:
            uri = res.log_model(mlf, paths)
        mlf.log_artifact(paths["scaler"])
        say(f" Logged run to MLflow experiment '{s.mlflow_experiment}' with input signature and examples")
        if summary["test_auc"] >= s.mlflow_auc_threshold:
            version = mlf.register_model(uri, s.mlflow_model_name)
            mlf.set_registered_model_alias(s.mlflow_model_name, s.mlflow_model_stage, version)
            say(f" Registered model version {version} (AUC {summary['test_auc']:.4f} >= {s.mlflow_auc_threshold}) "
                f"as models:/{s.mlflow_model_name}@{s.mlflow_model_stage}")
        else:
            say(f"i Model not registered (AUC {summary['test_auc']:.4f} < {s.mlflow_auc_threshold})")
        summary["run_id"] = run.info.run_id
    return version


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(description="Train the fraud model on MI355X (train_model.py)")
    ap.add_argument("--model", default=os.getenv("FDX_MODEL_TYPE", "logistic"), choices=["logistic", "gbdt"])
    ap.add_argument("--cv-folds", type=int, default=5)
    ap.add_argument("--model-dir", default="models")
    ap.add_argument("--json", default=None, help="write the run summary here")
    ap.add_argument("--checkpoint-dir", default=None,
                    help="resume directory: completed CV folds + GBDT tree checkpoints (FDX_CHECKPOINT_DIR)")
    ap.add_argument("--split", default=None, choices=["auto", "sklearn", "device"],
                    help="sklearn: reference-identical split; device: K3 kernel (default auto: device >= 2M rows on GPU)")
    ap.add_argument("--gbdt-eval-metric", default=None,
                    help="comma-separated logloss,error,auc,aucpr: per-round metrics of every CV fold on its own rows "
                         "(device GBDT CV job); the last one drives early stopping")
    ap.add_argument("--gbdt-early-stopping", type=int, default=None, metavar="N",
                    help="stop a fold after N rounds without improvement; the final fit grows "
                         "round(mean(best_iteration + 1)) trees")
    ap.add_argument("--gbdt-subsample", type=float, default=1.0,
                    help="row fraction every boosting round draws (stochastic boosting; 1.0: all rows)")
    ap.add_argument("--gbdt-colsample-bytree", type=float, default=1.0,
                    help="feature fraction every tree draws (1.0: all features)")
    ap.add_argument("--gbdt-seed", type=int, default=0, help="seed of the row / feature draws")
    ap.add_argument("--gbdt-monotone", default=None, metavar="NAME=SIGN,...",
                    help='monotone constraints by column name, e.g. "Amount=1,V14=-1": the score never falls (1) or '
                         "never rises (-1) as the column grows; an unknown name is an error")
    ap.add_argument("--gbdt-interaction", default=None, metavar="NAME,NAME;NAME,...",
                    help='interaction constraints by column name, e.g. "Amount,Time;V14,V17,V12": groups separated '
                         "by ';'; below a path of split columns a node may use those columns and every group that "
                         "contains them all; an unknown name is an error")
    ap.add_argument("--gbdt-reg-alpha", type=float, default=0.0,
                    help="L1 regularisation of the leaf weights (xgboost's reg_alpha; 0: off)")
    ap.add_argument("--gbdt-max-delta-step", type=float, default=0.0,
                    help="cap on a leaf weight's magnitude before the learning rate (xgboost's max_delta_step, its "
                         "advice for extremely imbalanced classes; 0: no cap)")
    ap.add_argument("--gbdt-cover", default=None, choices=["hessian", "count"],
                    help="store node covers over the real standardized training rows (not the SMOTE samples) in "
                         "xgb_model.json: hessian = xgboost's sum_hess, count = rows per node; the served model then "
                         "explains with path-dependent TreeSHAP (FDX_XAI_METHOD=tree_path) without a background file")
    a = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    comm = None
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:  # torchrun: one rank per GPU, RCCL (gloo on CPU)
        from .parallel.comm import Communicator

        dev = None
        if torch.cuda.is_available():
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
            dev = torch.device("cuda", torch.cuda.current_device())
        comm = Communicator(device=dev)
    try:
        over = {k: v for k, v in (("split", a.split), ("checkpoint_dir", a.checkpoint_dir)) if v}
        st = Settings.load(**over)
        out = run(st, model_type=a.model, cv_folds=a.cv_folds, model_dir=a.model_dir, comm=comm,
                  gbdt_eval_metric=a.gbdt_eval_metric.split(",") if a.gbdt_eval_metric else None,
                  gbdt_early_stopping=a.gbdt_early_stopping, gbdt_subsample=a.gbdt_subsample,
                  gbdt_colsample_bytree=a.gbdt_colsample_bytree, gbdt_seed=a.gbdt_seed,
                  gbdt_monotone=a.gbdt_monotone, gbdt_interaction=a.gbdt_interaction,
                  gbdt_reg_alpha=a.gbdt_reg_alpha, gbdt_max_delta_step=a.gbdt_max_delta_step,
                  gbdt_cover=a.gbdt_cover)
    finally:
        if comm is not None:
            comm.close()
    if comm is not None and comm.rank != 0:
        return 0
    if a.json:
        with open(a.json, "w") as f:
            json.dump({k: v for k, v in out.items() if k != "eval"} | {"eval": out["eval"]}, f, indent=1, default=str)
    return 0


if __name__ == "__main__":  # pragma: no cover
    raise SystemExit(main())


def tempdir() -> str:  # helper for scripts/tests
    return tempfile.mkdtemp(prefix="fdx_train_")
