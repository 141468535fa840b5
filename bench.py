#!/usr/bin/env python3
"""Flagship benchmark: BASELINE.json config 3 ("SMOTE k-NN + logistic SGD HIP train on one MI355X,
10M x 30 bf16, AUC >= 0.95"), scaled by data parallelism for configs 4/5.

One step = one complete training fit on every rank's shard, exactly the hot path of the
reference's train_model.py re-done on MI355X kernels:
    StandardScaler fit (K1, all-reduce) -> standardize/pad/cast to bf16 (K2, the same pass)
    -> SMOTE: minority all-gather, MFMA k-NN (K8), Philox interpolation folded into the passes (K9)
    -> LogisticRegression (C=1) by minibatch SGD to convergence (K4, the default --solver sgd:
       3 epochs of 4 / 6 / 6 minibatches, curvature-normalised heavy-ball steps, Polyak averaging,
       device-side convergence test on the epoch gradient, tol 1e-3; one persistent launch with a
       grid barrier per step on one GPU, one int64 all-reduce per step under DP), random-init weights.
    --solver newton: the same pipeline with the Newton fit (fused grad/loss/MFMA-Hessian pass, one
       1088-double all-reduce per iteration, on-device Cholesky) -- reported as an extra otherwise.
Weak scaling: every GPU owns ``--rows-per-gpu`` raw rows (80% train / 20% test, stratified by
construction), credit_card-shaped synthetic data (30 features, 0.17% fraud, Bayes AUC 0.970).

value = post-SMOTE training rows fitted per second, whole job (sum over ranks / slowest rank's
time).  Baseline = 3.50 M rows/s: sklearn lbfgs fit alone on the 10M-row post-SMOTE set
(our step additionally includes the scaler and SMOTE work).  A plain run sets up,
warms up, times the K steps and prints the result line.  With --full it then also reports, as
extra fields, the test AUC (exact, K10), the SGD fit's convergence state and objective against the
Newton optimum on the same training set, the other solver / row formats, and the LinearSHAP /
KernelSHAP throughputs.  --dump-outputs DIR writes what the last timed fit returned (weights,
scaler parameters, row counts) as DIR/<name>.npy; the inputs are seeded, so two builds can be
compared array for array.

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]
       torchrun --nproc-per-node N bench.py --gpus N ...
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

BASELINE_TRAIN_ROWS_PER_S = 3.50e6      # 15.97M post-SMOTE rows in 4.56 s
BASELINE_LINEAR_SHAP_PER_S = 316e6      # BASELINE.md §2, LinearSHAP values/s at 10M
# CPU KernelSHAP (config 4's missing CPU baseline): shap's algorithm as vectorised fp64 numpy on this
# image's 8-core EPYC, 2042 coalitions x 100 background rows (tools/cpu_kernelshap_baseline.py,
# profiles/r2_s3k/cpu_kernelshap_baseline.json)
BASELINE_CPU_KERNELSHAP_PER_S = 4671.3


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows-per-gpu", type=int, default=10_000_000)
    ap.add_argument("--solver", default="sgd", choices=["newton", "sgd"],
                    help="sgd: config 3's solver (the headline); newton: the Newton fit")
    ap.add_argument("--storage", default="bf16", choices=["bf16", "fp8"])
    ap.add_argument("--smote-scope", default="auto", choices=["auto", "global", "shard"],
                    help="SMOTE under DP: global = exactly the single-process SMOTE, the reference's "
                         "semantics (every rank a slice of one draw sequence over all minority rows; "
                         "exact k-NN over all of them, so per-rank k-NN work grows with N); shard = "
                         "per-partition SMOTE (constant per-rank work). auto: the headline uses global "
                         "and a DP run with --full ALSO times the shard scope, reported as shard_scope")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the extra measurements (test AUC, convergence "
                         "against Newton, the other solvers / row formats, CV jobs, SHAP, predict, GBDT); "
                         "a plain run times the headline fit only")
    ap.add_argument("--no-extras", action="store_true",
                    help="deprecated: a run without --full is already headline only (still accepted "
                         "for older command lines; overrides --full)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed fit returned as DIR/<name>.npy (float64)")
    ap.add_argument("--json-out", default=None)
    return ap.parse_args(argv)


def _wants_extras(args, cpu_mode: bool) -> bool:
    """The extra measurements run only on request (--full), never in the CPU contract mode."""
    return bool(args.full) and not args.no_extras and not cpu_mode


def _dump_outputs(res, path: str) -> None:
    """The last timed fit's result, as a caller of DevicePipeline.fit receives it: the
    standardized-space weights (w[30] = intercept), the scaler's parameters and the row counts.
    About 1 KB in all; the inputs are seeded, so two builds compare array for array."""
    os.makedirs(path, exist_ok=True)
    mean, var, scale = res.scaler.numpy()
    arrays = {
        "weights": res.w, "coef": res.coef, "intercept": [res.intercept],
        "scaler_mean": mean, "scaler_var": var, "scaler_scale": scale,
        "row_counts": [res.n_rows, res.n_train_rows, res.n_minority, res.n_synthetic],
    }
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def _free_port() -> int:
    import socket

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _self_launch(args) -> int:
    """``python bench.py --gpus N`` with no torchrun around it: start N ranks (one process per
    GPU, RCCL over xGMI) as CHILD processes via torch.distributed.run and exit with their status.
    Nothing in this parent touches the GPU (no torch.cuda call before the children exist), and the
    parent is never replaced by exec -- it waits for the launcher and forwards its exit code (the
    launcher tears every rank down when one fails)."""
    import subprocess

    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL peer buffers on this driver
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.abspath(__file__)] + sys.argv[1:]
    print(f"[bench] self-launch: {args.gpus} ranks via torch.distributed.run", file=sys.stderr, flush=True)
    rc = subprocess.call(cmd, env=env)
    return 0 if rc == 0 else (rc if rc > 0 else 1)


def _cpu_mode() -> bool:
    """FDX_BENCH_DEVICE=cpu: the same code path on CPU tensors over gloo -- the CPU test of the
    launch / rank / JSON contract (never a performance number)."""
    return os.environ.get("FDX_BENCH_DEVICE", "cuda") == "cpu"


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def main():
    args = parse()
    world_env = os.environ.get("WORLD_SIZE")
    if world_env is None and args.gpus > 1:
        return _self_launch(args)
    world_env = int(world_env or "1")
    if world_env != args.gpus:
        print(f"[bench] FATAL: --gpus {args.gpus} but WORLD_SIZE={world_env}: the launcher and the "
              "requested GPU count disagree", file=sys.stderr, flush=True)
        return 2

    from fraud_detection_amd.data.synthetic import separable
    from fraud_detection_amd.models.pipeline import DevicePipeline, TrainConfig, evaluate
    from fraud_detection_amd.parallel.comm import Communicator

    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if _cpu_mode():
        dev = torch.device("cpu")
        comm = Communicator(backend="gloo") if world_env > 1 else None
    else:
        if not torch.cuda.is_available():
            print("bench.py requires a ROCm GPU (FDX_BENCH_DEVICE=cpu for the CPU contract test)", file=sys.stderr)
            return 2
        # Rehearsal knobs for a one-GPU box (never used by the driver's runs): FDX_BENCH_ONE_GPU=1
        # puts every rank on cuda:0, FDX_BENCH_BACKEND=gloo swaps RCCL for host-staged gloo.
        if os.environ.get("FDX_BENCH_ONE_GPU") == "1":
            local_rank = 0
        elif local_rank >= torch.cuda.device_count():
            print(f"[bench] FATAL: LOCAL_RANK {local_rank} but only {torch.cuda.device_count()} GPUs visible",
                  file=sys.stderr, flush=True)
            return 2
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
        comm = Communicator(backend=os.environ.get("FDX_BENCH_BACKEND") or None, device=dev) if world_env > 1 else None
    rank = comm.rank if comm else 0
    world = comm.world_size if comm else 1
    if world != args.gpus:
        raise SystemExit(f"[bench] FATAL: communicator world {world} != --gpus {args.gpus}")

    n_total = args.rows_per_gpu
    n_test = n_total // 5
    n_train = n_total - n_test
    X, y = separable(n_train, seed=1000 + rank, device=dev)
    want_extras = _wants_extras(args, _cpu_mode())
    if want_extras:  # the test split: only the extras evaluate on it
        Xt, yt = separable(n_test, seed=5000 + rank, device=dev)

    scope = args.smote_scope if args.smote_scope != "auto" else "global"
    cfg = TrainConfig(solver=args.solver, storage=args.storage, seed=42, smote_scope=scope)
    pipe = DevicePipeline(cfg, comm)

    def step():
        # random-init weights each fit (reference model family, no checkpoint)
        return pipe.fit(X, y)

    res = None
    for _ in range(args.warmup):
        res = step()
    pipe.settle()
    if comm:
        comm.barrier()
    _sync(dev)
    if comm:
        comm.stats.reset()  # the per-collective breakdown covers the timed steps only
    # device-side step boundaries (hipEvent times): an event behind every fit's
    # last kernel on the compute stream; the host runs ahead, so event i -> i+1 spans exactly
    # fit i+1's kernels and any device idle in front of them
    # FDX_BENCH_EVENTS=0 (lab): no per-fit events, wall clock only (isolates the events' own cost)
    use_ev = dev.type == "cuda" and os.environ.get("FDX_BENCH_EVENTS", "1") != "0"
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)] if use_ev else None
    t0 = time.perf_counter()
    if ev:
        ev[0].record()
    for i in range(args.steps):
        res = step()
        if ev:
            ev[i + 1].record()
    pipe.settle()  # every deferred convergence check of the timed fits resolves inside the region
    _sync(dev)
    if comm:
        comm.barrier()
    elapsed = time.perf_counter() - t0
    if comm:
        elapsed = comm.max_over_ranks(elapsed)
    ms_per_step = 1000.0 * elapsed / max(args.steps, 1)
    step_ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps)] if ev else [ms_per_step] * args.steps
    med_ms, max_ms = float(np.median(step_ms)), float(np.max(step_ms))
    if comm:
        med_ms, max_ms = comm.max_over_ranks(med_ms), comm.max_over_ranks(max_ms)
    coll = comm.collective_summary() if comm else {}
    rows_local = res.n_train_rows
    rows_global = comm.all_reduce_scalar(float(rows_local)) if comm else float(rows_local)
    raw_global = comm.all_reduce_scalar(float(n_train)) if comm else float(n_train)
    value = rows_global / (ms_per_step / 1000.0)

    if args.dump_outputs and rank == 0:
        _dump_outputs(res, args.dump_outputs)

    extras = {}
    if want_extras:
        ev = evaluate(res, Xt, yt, comm)
        extras["auc"] = round(ev["auc"], 6)
        extras["confusion"] = {k: ev[k] for k in ("tn", "fp", "fn", "tp")}
        extras["newton_iters" if args.solver == "newton" else "sgd_steps"] = res.fit.n_iter
        extras["fit_converged"] = res.fit.converged
        if args.solver == "sgd" and comm is None:
            extras["sgd"] = _sgd_details(pipe, res, X, y, scope, args.storage)
        prof = pipe.fit(X, y, profile=True)
        extras["phase_ms"] = {k: round(v * 1000, 3) for k, v in prof.timings.items()}
        extras.update(_shap_throughput(res, dev, comm))
        extras.update(_variants(args, X, y, Xt, yt, dev, comm, scope))
        if comm is not None:  # both scopes in one line: the other scope as an extra
            from fraud_detection_amd.models.pipeline import DevicePipeline as _DP, TrainConfig as _TC

            other = "shard" if scope == "global" else "global"
            gpipe = _DP(_TC(solver=args.solver, storage=args.storage, seed=42, smote_scope=other), comm)
            gr, gdt = _timed_fits(gpipe, X, y, dev, comm)
            grows = comm.all_reduce_scalar(float(gr.n_train_rows))
            extras[f"{other}_scope"] = {
                "ms_per_step": round(gdt * 1e3, 4), "rows_per_sec": round(grows / gdt, 1),
                "auc": round(evaluate(gr, Xt, yt, comm)["auc"], 6),
                "note": ("per-partition SMOTE: neighbours within a rank's shard (constant per-rank work)"
                         if other == "shard" else
                         "exact single-process SMOTE semantics; k-NN over all ranks' minority rows")}
        extras.update(_end_to_end(X, y, Xt, yt, cfg, dev, comm))
        if comm is None:
            extras.update(_cv_job(X, y, Xt, yt, args, ms_per_step))
        extras.update(_worker_kernelshap(res, X, dev, comm))
        extras.update(_batch_predict(res, dev, comm))
        if comm is None:
            extras.update(_knn_dp8_projection(res, X, y, dev))
        extras.update(_gbdt(X, y, Xt, yt, dev, comm))
    out = {
        "metric": "train_rows_per_sec (SMOTE k-NN + logistic fit, post-SMOTE rows/s, whole job); AUC; SHAP values/s",
        "value": round(value, 1),
        "unit": "rows/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4),
        "ms_per_step_median": round(med_ms, 4),
        "ms_per_step_max": round(max_ms, 4),
        "timing": "wall clock of K back-to-back fits between barrier+synchronize (pending checks settled "
                  "inside); median/max from hipEvents at the fit boundaries on the compute stream",
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": round(value / BASELINE_TRAIN_ROWS_PER_S, 2),
        "dtype": args.storage,
        "data": "synthetic credit_card-shaped (30 feat, 0.17% fraud, delta=2.66), random-init weights",
        "config": {
            "model": f"StandardScaler+SMOTE(k=5)+LogisticRegression(C=1,{args.solver})",
            "global_batch": int(raw_global),
            "seq_len": 30,
            "parallelism": f"dp{world}",
            "rows_per_gpu": args.rows_per_gpu,
            "post_smote_rows_global": int(rows_global),
            "smote_scope": scope,
        },
    }
    if coll:
        out["collectives_timed_region"] = {k: v for k, v in coll.items()}
    out.update(extras)
    if rank == 0:
        # every measured variant must reach BASELINE's AUC target: a number from a wrong model is
        # not a measurement (stderr, so the one-line JSON contract is unchanged)
        aucs = {"headline": out.get("auc")}
        aucs.update({k: v.get("auc") for k, v in out.items() if isinstance(v, dict) and "auc" in v})
        low = {k: v for k, v in aucs.items() if v is not None and v < 0.95}
        if low:
            print(f"[bench] WARNING: AUC below the 0.95 target: {low}", file=sys.stderr, flush=True)
        line = json.dumps(out)
        print(line, flush=True)
        if args.json_out:
            with open(args.json_out, "w") as f:
                f.write(line + "\n")
    if comm:
        comm.close()
    return 0


def _timed_fits(pipe, X, y, dev, comm, reps=3, warmup=1):
    for _ in range(max(warmup, 1)):
        pipe.fit(X, y)
    pipe.settle()
    if comm:
        comm.barrier()
    torch.cuda.synchronize(dev)
    # events at the fit boundaries on the compute stream (as the headline's median): a fit that
    # stalls shows in the mean and the max, not in the median
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    t0 = time.perf_counter()
    r = None
    ev[0].record()
    for i in range(reps):
        r = pipe.fit(X, y)
        ev[i + 1].record()
    pipe.settle()
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / reps
    med = float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(reps)])) * 1e-3
    if comm:
        dt, med = comm.max_over_ranks(dt), comm.max_over_ranks(med)
    _timed_fits.last_median = med
    return r, dt


def _variants(args, X, y, Xt, yt, dev, comm, scope) -> dict:
    """The other solver and row formats (config 5 names fp8 rows): ms/fit + AUC of each variant in
    the same run (the headline step above is config 3's bf16 SGD fit by default)."""
    from fraud_detection_amd.models.pipeline import DevicePipeline, TrainConfig, evaluate

    out = {}
    # *_stored_smote: the fit with its SMOTE rows written and streamed (the default folds them into
    # the passes instead: TrainConfig.virtual_smote)
    for name, kw in (("newton_bf16", dict(solver="newton", storage="bf16")),
                     ("sgd_bf16", dict(solver="sgd", storage="bf16")), ("newton_fp8", dict(solver="newton", storage="fp8")),
                     ("newton_bf16_stored_smote", dict(solver="newton", storage="bf16", virtual_smote=False)),
                     ("newton_fp8_stored_smote", dict(solver="newton", storage="fp8", virtual_smote=False)),
                     ("sgd_fp8", dict(solver="sgd", storage="fp8"))):
        if kw["solver"] == args.solver and kw["storage"] == args.storage and kw.get("virtual_smote", True):
            continue
        pipe = DevicePipeline(TrainConfig(seed=42, smote_scope=scope, **kw), comm)
        # the headline's own --steps / --warmup: variant numbers as stable as the headline's
        r, dt = _timed_fits(pipe, X, y, dev, comm, reps=max(args.steps, 1), warmup=args.warmup)
        rows = comm.all_reduce_scalar(float(r.n_train_rows)) if comm else float(r.n_train_rows)
        o = {"ms_per_fit": round(dt * 1e3, 4), "ms_per_fit_median": round(_timed_fits.last_median * 1e3, 4),
             "rows_per_sec": round(rows / dt, 1),
             "auc": round(evaluate(r, Xt, yt, comm)["auc"], 6)}
        if kw["solver"] == "sgd" and comm is None:
            o.update(_sgd_details(pipe, r, X, y, scope, kw["storage"]))
        out[name] = o
    return out


_NEWTON_W = {}


def _sgd_details(pipe, r, X, y, scope, storage) -> dict:
    """Config 3's solver: its device convergence state and its exact training objective against the
    Newton optimum on the SAME training set (same rows and SMOTE samples).  Call right after the
    fit (the objective is evaluated over the pipeline's current training buffer)."""
    from fraud_detection_amd.models.pipeline import DevicePipeline, TrainConfig

    if storage not in _NEWTON_W:
        npipe = DevicePipeline(TrainConfig(seed=42, smote_scope=scope, storage=storage, deferred_check=False))
        _NEWTON_W[storage] = npipe.fit(X, y).w
    f = r.fit
    mine = pipe.training_objective(r)
    opt = pipe.training_objective(r, w=_NEWTON_W[storage])
    return dict(steps=int(f.n_iter), epochs=pipe.cfg.sgd_epochs,
                minibatches_per_epoch=[int(v) for v in pipe.cfg.sgd_epoch_batches[:pipe.cfg.sgd_epochs]],
                extra_epoch_minibatches=[int(v) for v in pipe.cfg.sgd_epoch_batches[pipe.cfg.sgd_epochs:]],
                converged=bool(f.converged), epoch_grad_max=float(f.grad_max), tol=pipe.cfg.sgd_tol,
                recovered_launch=bool(getattr(f, "recovered", False)),
                objective=round(mine["objective"], 9), newton_objective=round(opt["objective"], 9),
                objective_rel_gap_vs_newton=float((mine["objective"] - opt["objective"]) / opt["objective"]),
                virtual_smote=pipe._virtual is not None)


def _end_to_end(X, y, Xt, yt, cfg, dev, comm) -> dict:
    """BASELINE.md §3 end-to-end pipeline: raw rows in host memory (the parsed CSV, pinned) ->
    upload -> scaler + SMOTE + fit -> exact test AUC, wall clock of the whole chain."""
    from fraud_detection_amd.models.pipeline import DevicePipeline, evaluate

    Xh, yh = X.cpu().pin_memory(), y.cpu().pin_memory()
    Xth, yth = Xt.cpu().pin_memory(), yt.cpu().pin_memory()
    pipe = DevicePipeline(cfg, comm)

    def chain():
        Xd, yd = Xh.to(dev, non_blocking=True), yh.to(dev, non_blocking=True)
        Xtd, ytd = Xth.to(dev, non_blocking=True), yth.to(dev, non_blocking=True)
        r = pipe.fit(Xd, yd)
        return evaluate(r, Xtd, ytd, comm)["auc"]

    chain()
    if comm:
        comm.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        auc = chain()
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / reps
    if comm:
        dt = comm.max_over_ranks(dt)
    raw = float(X.shape[0] + Xt.shape[0])
    raw = comm.all_reduce_scalar(raw) if comm else raw
    return {"end_to_end": {"ms": round(dt * 1e3, 3), "raw_rows_per_sec": round(raw / dt, 1), "auc": round(auc, 6),
                           "includes": "host->device upload of raw train+test rows, scaler, SMOTE, fit, exact AUC"}}


def _cv_job(X, y, Xt, yt, args, single_ms) -> dict:
    """The reference's whole training job (train_model.py:36-110) at the bench shape: one scaler on
    the training split, 5-fold stratified CV with SMOTE inside every fold, the final fit on the
    whole split, 5 fold AUCs + the test AUC -- models/cv.DeviceCV on the fold-sorted device table
    (no per-fold copies).  Per-fold times are hipEvents on the compute stream."""
    from fraud_detection_amd.models.cv import DeviceCV
    from fraud_detection_amd.models.pipeline import TrainConfig

    out = {}
    for solver, warm in (("newton", True), ("sgd", True), ("newton", False)):
        cv = DeviceCV(TrainConfig(solver=solver, storage=args.storage, seed=42), warm_start=warm)
        cv.run(X, y, Xt, yt)  # warm-up: allocations, first-touch
        best = None
        for _ in range(3):
            r = cv.run(X, y, Xt, yt)
            if best is None or r.total_ms < best.total_ms:
                best = r
        r = best
        key = "cv_job" if solver == args.solver else f"cv_job_{solver}"
        if solver == "newton" and not warm:
            key = "cv_job_newton_cold"  # every fold fitted from the random init, like the reference
        out[key] = {
            "ms": round(r.total_ms, 3), "x_single_fit": round(r.total_ms / single_ms, 2) if solver == args.solver else None,
            "device_ms": {"prep": round(r.prep_ms, 3), "folds": [round(t, 3) for t in r.fold_ms],
                          "final_fit": round(r.final_ms, 3)},
            "fold_aucs": [round(a, 6) for a in r.fold_aucs], "cv_auc_mean": round(r.cv_auc_mean, 6),
            "test_auc": round(r.test_auc, 6), "fold_iters": r.fold_iters,
            "includes": "fold codes + fold permutation + one scatter-form scaler pass, 5 x (k-NN, SMOTE "
                        "buckets, fit, validation logits, exact AUC), final fit, test AUC; best of 3 wall clock"}
    return out


def _worker_kernelshap(res, X, dev, comm) -> dict:
    """BASELINE config 4 as the async worker runs it: InferenceEngine.explain on a 1k-explanation
    lease from host memory (upload, predict, KernelSHAP MFMA coalition GEMM, download)."""
    from fraud_detection_amd.compat.sklearn_export import LinearArtifacts
    from fraud_detection_amd.serve.engine import InferenceEngine, sample_background

    mean, var, scale = res.scaler.numpy()
    art = LinearArtifacts(coef=res.coef, intercept=res.intercept, mean=mean, var=var, scale=scale,
                          n_samples_seen=int(res.scaler.n), feature_names=[f"f{i}" for i in range(len(mean))])
    Xh = X[:200_000].cpu().numpy()
    eng = InferenceEngine(art, device=dev, background=sample_background(Xh, 100))
    lease = Xh[1000:2000]
    for _ in range(3):
        eng.explain(lease, "kernel")
    if comm:
        comm.barrier()
    t0 = time.perf_counter()
    reps = 10
    for _ in range(reps):
        ex = eng.explain(lease, "kernel")
    dt = (time.perf_counter() - t0) / reps
    if comm:
        dt = comm.max_over_ranks(dt)
    world = comm.world_size if comm else 1
    err = float(abs(ex.phi.sum(1) - (ex.prob - ex.base_value)).max())
    return {"kernelshap_worker_values_per_sec": round(1000 * 30 * world / dt, 1),
            "kernelshap_worker": {"explanations_per_lease": 1000, "ms_per_lease": round(dt * 1e3, 3),
                                  "efficiency_max_err": err, "per_gpu_worker_processes": world}}


def _batch_predict(res, dev, comm) -> dict:
    """BASELINE config 2 (batch /predict, 1M x 30, reference consumer evaluate_model.py:26-27):
      * bf16 rows: the predict kernel over 1M standardized bf16 training-layout rows;
      * raw fused: scaler folded into the GEMV, raw fp32 rows in HBM (one kernel);
      * host to host: InferenceEngine.predict_proba on 1M raw rows in host memory -> fp64 scores in
        host memory (rows page-locked in place, H2D | kernel | D2H pipelined; output arrays reused
        like a batch-scoring loop would)."""
    from fraud_detection_amd.compat.sklearn_export import LinearArtifacts
    from fraud_detection_amd.data.synthetic import separable
    from fraud_detection_amd.ops import predict as P
    from fraud_detection_amd.ops import scaler as S
    from fraud_detection_amd.serve.engine import InferenceEngine

    n = 1_000_000
    Xq, _ = separable(n, seed=91, device=dev)
    rows = torch.empty((n, 32), dtype=torch.bfloat16, device=dev)
    S.scale_cast(Xq, res.scaler, out=rows)
    # resident device weights (a serving loop holds them on the device): no copy, no read-back
    w = torch.from_numpy(res.w).to(dev, torch.float32)
    a, c, b = res.folded()
    at, ct = torch.from_numpy(a).to(dev, torch.float32), torch.from_numpy(c).to(dev, torch.float32)
    prob = torch.empty(n, dtype=torch.float32, device=dev)

    def dev_rate(fn, reps=50):
        """Device time per call from hipEvents around `reps` back-to-back launches (the launches
        queue ahead of the GPU, so this is kernel time plus the kernel boundaries)."""
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    nat = P.native()
    s = torch.cuda.current_stream(dev).cuda_stream
    t_bf16 = dev_rate(lambda: nat.predict_bf16(rows.data_ptr(), n, w.data_ptr(), prob.data_ptr(), 0, s))
    t_bf16_api = dev_rate(lambda: P.predict_rows(rows, w))
    t_raw = dev_rate(lambda: P.predict_shap_raw(Xq, at, ct, b, dphi=0))
    mean, var, scale = res.scaler.numpy()
    eng = InferenceEngine(LinearArtifacts(coef=res.coef, intercept=res.intercept, mean=mean, var=var, scale=scale,
                                          n_samples_seen=int(res.scaler.n), feature_names=[f"f{i}" for i in range(30)]),
                          device=dev)
    Xh = Xq.cpu().numpy()
    out = (np.empty(n), np.empty(n))
    for _ in range(3):
        eng.predict_proba(Xh, out=out)
    reps = 10
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.predict_proba(Xh, out=out)
    t_h2h = (time.perf_counter() - t0) / reps
    world = comm.world_size if comm else 1
    if comm:
        t_bf16, t_bf16_api, t_raw, t_h2h = (comm.max_over_ranks(t) for t in (t_bf16, t_bf16_api, t_raw, t_h2h))
    return {"predict_1M_bf16_rows_per_sec": round(n * world / t_bf16, 1),
            "predict_1M": {"bf16_rows_kernel_us": round(t_bf16 * 1e6, 2),
                           "bf16_rows_tb_per_s": round(n * 64 / t_bf16 / 1e12, 2),
                           "bf16_predict_rows_api_us": round(t_bf16_api * 1e6, 2),
                           "timing": "hipEvents around 50 back-to-back launches, resident fp32 device weights",
                           "raw_fused_kernel_us": round(t_raw * 1e6, 2),
                           "raw_fused_rows_per_sec": round(n * world / t_raw, 1),
                           "host_to_host_ms": round(t_h2h * 1e3, 3),
                           "host_to_host_rows_per_sec": round(n * world / t_h2h, 1),
                           "vs_cpu_predict_proba_25.7M": round(n / t_h2h / 25.7e6, 2)},
            "predict_1M_host_to_host_ms": round(t_h2h * 1e3, 3)}


def _knn_dp8_projection(res, X, y, dev) -> dict:
    """Global-scope SMOTE under DP=8 (the single-process SMOTE semantics): every rank queries its
    own minority rows against ALL ranks' minority rows, so per-rank k-NN work grows with N while the
    other phases stay constant (weak scaling).  Measured here on one GPU with the real kernels:
    this rank's minority rows against the minority rows of 8 shards (this one + 7 more generated
    exactly as ranks 1..7 of an 8-GPU run would generate theirs)."""
    from fraud_detection_amd.data.synthetic import separable
    from fraud_detection_amd.ops import knn as K
    from fraud_detection_amd.ops import scaler as S

    def minority(Xs, ys):
        idx = S.compact_indices(ys, 1)
        return S.scale_cast(Xs, res.scaler, labels=ys, out_dtype="f32", idx=idx)

    q = minority(X, y)
    shards = [q]
    for r in range(1, 8):
        Xr, yr = separable(X.shape[0], seed=1000 + r, device=dev)
        shards.append(minority(Xr, yr))
        del Xr, yr
    C = torch.cat(shards)

    def t(Cand, reps=20):
        for _ in range(3):
            K.knn_topk(q, Cand, k=5, self_offset=0)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(reps):
            K.knn_topk(q, Cand, k=5, self_offset=0)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / reps

    t1, t8 = t(q), t(C)
    return {"dp8_global_scope_knn_projection": {
        "queries_per_rank": int(q.shape[0]), "candidates_dp1": int(q.shape[0]), "candidates_dp8": int(C.shape[0]),
        "knn_ms_dp1": round(t1 * 1e3, 4), "knn_ms_dp8_per_rank": round(t8 * 1e3, 4),
        "note": "per-rank k-NN time at DP=8 global scope (queries = this rank's minority rows)"}}


def _gbdt(X, y, Xt, yt, dev, comm) -> dict:
    """The reference's own model family (train_model.py:69-106: XGBoost, 100 trees, depth 5,
    eta 0.1) on the bench rows after SMOTE: boosting time, per-tree time and test AUC."""
    from fraud_detection_amd.models.gbdt import GBDTPipeline
    from fraud_detection_amd.models.pipeline import TrainConfig
    from fraud_detection_amd.ops import gbdt as gb

    GBDTPipeline(TrainConfig(), gb.GBDTParams(n_estimators=2), comm=comm).fit(X, y)  # warm-up
    if comm:
        comm.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    r = GBDTPipeline(TrainConfig(), gb.GBDTParams(n_estimators=100, max_depth=5, learning_rate=0.1), comm=comm).fit(X, y)
    torch.cuda.synchronize(dev)
    fit_s = time.perf_counter() - t0
    boost_s = r.timings["boost"]
    if comm:
        fit_s, boost_s = comm.max_over_ranks(fit_s), comm.max_over_ranks(boost_s)
    ev = r.evaluate(Xt, yt, comm)
    out = {"gbdt": {"trees": 100, "depth": 5, "post_smote_rows": int(r.n_train_rows), "fit_ms": round(fit_s * 1e3, 2),
                    "ms_per_tree": round(boost_s * 1e3 / 100, 3), "auc": round(ev["auc"], 6),
                    "scale_pos_weight": round(r.scale_pos_weight, 4)}}
    if comm is None:
        out.update(_gbdt_cv_job(X, y, Xt, yt, fit_s * 1e3))
    return out


def _gbdt_cv_job(X, y, Xt, yt, single_fit_ms) -> dict:
    """The reference's actual training job (train_model.py:49-110: XGB, 5-fold CV with SMOTE inside
    every fold, final fit, test AUC) as models/gbdt_cv.DeviceGBDTCV: one binned fold-sorted table,
    folds fit around their own block (no per-fold copies), validation scores from the rounds'
    margin walk.  Device ms per fold from hipEvents."""
    from fraud_detection_amd.models.gbdt_cv import DeviceGBDTCV
    from fraud_detection_amd.models.pipeline import TrainConfig
    from fraud_detection_amd.ops import gbdt as gb

    cv = DeviceGBDTCV(TrainConfig(), gb.GBDTParams(n_estimators=100, max_depth=5, learning_rate=0.1))
    r = cv.run(X, y, Xt, yt)
    return {"gbdt_cv_job": {
        "ms": round(r.total_ms, 2), "x_single_fit": round(r.total_ms / single_fit_ms, 2),
        "device_ms": {"prep": round(r.prep_ms, 2), "folds": [round(t, 2) for t in r.fold_ms],
                      "final_fit": round(r.final_ms, 2)},
        "fold_aucs": [round(a, 6) for a in r.fold_aucs], "cv_auc_mean": round(r.cv_auc_mean, 6),
        "test_auc": round(r.test_auc, 6), "fold_rows": r.fold_rows,
        "includes": "fold codes + permutation + scaler + one quantile pass + binned fold-sorted table, 5 x (k-NN, "
                    "SMOTE generate + bin into the table tail, 100 trees around the fold's block, exact AUC of "
                    "the block's margins), final fit, test AUC; wall clock"}}


def _shap_throughput(res, dev, comm) -> dict:
    """LinearSHAP (fused predict + attributions, raw fp32 in) on 1M rows per GPU, and the
    KernelSHAP coalition-GEMM worker path (1k explanations) when its kernel is present."""
    from fraud_detection_amd.data.synthetic import separable
    from fraud_detection_amd.ops import predict as P

    out = {}
    Xs, _ = separable(1_000_000, seed=77, device=dev)
    a, c, b = res.folded()
    at, ct = torch.from_numpy(a).to(dev), torch.from_numpy(c).to(dev)
    for _ in range(3):
        P.predict_shap_raw(Xs, at, ct, b)
    reps = 20
    if comm:
        comm.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        P.predict_shap_raw(Xs, at, ct, b)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    if comm:
        dt = comm.max_over_ranks(dt)
    world = comm.world_size if comm else 1
    vals = 1_000_000 * 30 * reps * world / dt
    out["linear_shap_values_per_sec"] = round(vals, 1)
    out["linear_shap_vs_baseline"] = round(vals / BASELINE_LINEAR_SHAP_PER_S, 2)
    try:
        from fraud_detection_amd.models.explainers import kernelshap_throughput

        out.update(kernelshap_throughput(res, dev, comm))
        out["kernelshap_vs_cpu_kernelshap"] = round(out["kernelshap_values_per_sec"] / BASELINE_CPU_KERNELSHAP_PER_S, 1)
    except (ImportError, AttributeError):
        pass
    return out


if __name__ == "__main__":
    sys.exit(main())
