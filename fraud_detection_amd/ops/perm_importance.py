"""Permutation feature importance of a tree ensemble's margin (csrc/kernels/tree_perm.hip): the
per-feature mask words, the device wrappers and the CPU path (the numpy oracle of
ops/reference_gbdt.py).

Column (feature f, repeat r) gives row i feature f of row ``permutation_donors(n, seed, f, r)[i]``
and leaves the rest of the row as observed.  A row's directions in a tree are one 32-bit word (bit
k: heap node k sends the row right) and the substitution only changes the bits of the nodes that
split on f: ``feature_masks(ens)[t, f]`` has those nodes' bits (the ``mask`` of
ops/pdp.override_words, for every feature at once), and the kernel takes the donor's comparison
there and the row's own bit everywhere else.  Every column's margins are then scored by the exact
integer metric kernels (auc_radix, the precision-recall kernels, gbdt_eval) on the same stream into
one int64 table that is read back once."""
from __future__ import annotations

import numpy as np
import torch

from . import reference_gbdt as R
from .native import native, ptr, stream_of

SCORINGS = ("auc", "aucpr", "logloss")
DEFAULT_MAX_BYTES = 256 << 20


def feature_masks(ens) -> np.ndarray:
    """uint32 [T, 32]: bit k of [t, f] is set where heap node k (1-based) of tree t splits on
    feature f.  A pass-through node (feat -1) is in no mask."""
    T, ni = ens.feat.shape
    out = np.zeros((T, 32), np.uint32)
    rows = np.arange(T)
    for n in range(ni):
        f = ens.feat[:, n]
        on = f >= 0
        out[rows[on], f[on]] |= np.uint32(2 << n)
    return out


def _check_rows(X: torch.Tensor, expl):
    if X.dim() != 2 or X.dtype != torch.float32 or X.shape[1] != expl.d or (X.shape[0] and X.stride(1) != 1):
        raise ValueError(f"X must be float32 [n, {expl.d}] with unit column stride")


def _device_ensemble(expl, dev):
    """The explainer's ensemble and scaler on the device (ops/pdp's per-device cache) with the mask
    words beside them."""
    from .pdp import _device_design

    t = _device_design(expl, dev)
    if "fmask" not in t:
        t["fmask"] = torch.from_numpy(feature_masks(expl.ens).view(np.int32)).to(dev)
    return t


def _launch(Xs, t, ens, d, cols, seed, out):
    """Enqueue tree_perm for the columns ``cols`` = [(f, r)] into out [len(cols), n]."""
    n = int(Xs.shape[0])
    dev = Xs.device
    cf = torch.tensor([c[0] for c in cols], dtype=torch.int32).to(dev)
    cr = torch.tensor([c[1] for c in cols], dtype=torch.int32).to(dev)
    native().tree_perm(ptr(Xs), n, Xs.stride(0), d, ptr(t["feat"]), ptr(t["thr"]), ptr(t["leaf"]), ptr(t["dleft"]),
                       ptr(t["fmask"]), ens.n_trees, ens.depth, float(ens.base_margin), ptr(cf), ptr(cr), len(cols),
                       int(seed), ptr(out), stream_of(Xs))


def permuted_margins(X: torch.Tensor, expl, features=None, n_repeats: int = 5, seed: int = 0, sync: bool = True):
    """(float32 [F, R, n] permuted margins, float32 [n] baseline) of ``expl`` (a
    TreePermutationImportance) over the RAW fp32 rows X [n, d] (unit column stride, any row stride;
    standardized with the explainer's scaler, a NaN stays NaN and follows default_left, whether it
    is the row's own or the donor's).  [i, r] is bit for bit ``predict_margin`` on the rows whose
    feature ``features[i]`` is permuted by ``permutation_donors(n, seed, features[i], r)``.  Device
    rows run csrc/kernels/tree_perm.hip in ONE launch (numpy results if ``sync`` else device
    tensors); CPU rows run the oracle."""
    ens = expl.ens
    _check_rows(X, expl)
    fs = R.perm_check(ens, features, n_repeats, seed)
    n, F, Rn = int(X.shape[0]), len(fs), int(n_repeats)
    if not X.is_cuda:
        from ..models.explainers import _standardize

        pm, base = R.permuted_margins_reference(_standardize(X.numpy(), expl.mean, expl.scale), ens, fs, Rn, seed)
        return (pm, base) if sync else (torch.from_numpy(pm), torch.from_numpy(base))
    from .scaler import scale_cast

    dev = X.device
    out = torch.empty((F * Rn + 1, n), dtype=torch.float32, device=dev)
    if n:
        t = _device_ensemble(expl, dev)
        Xs = scale_cast(X, t["stats"], out_dtype="f32")
        _launch(Xs, t, ens, expl.d, [(f, r) for f in fs for r in range(Rn)] + [(-1, 0)], seed, out)
    pm, base = out[:-1].view(F, Rn, n), out[-1]
    return (pm.cpu().numpy(), base.cpu().numpy()) if sync else (pm, base)


def _raw_of_record(scoring: str, rec):
    """(raw, positives, rows) of one row of the int64 score table."""
    if scoring == "logloss":                      # gbdt_eval: (loss_q, n_err, n_pos, n_rows)
        return int(rec[0]), int(rec[2]), int(rec[3])
    return int(rec[0]), int(rec[1]), int(rec[1]) + int(rec[2])   # (twice_pairs | ap_q, P, N, ..)


def permutation_scores(X: torch.Tensor, y: torch.Tensor, expl, features=None, scoring: str = "auc",
                       n_repeats: int = 5, seed: int = 0, max_bytes: int = DEFAULT_MAX_BYTES):
    """(raw int64 [F, R], baseline_raw int, positives int): every permuted column's margins and the
    baseline's, scored against the 0/1 labels y [n] (uint8, on X's device) as the exact integer of
    the metric kernel -- "auc": twice_pairs (auc_radix; AUC = raw / (2 P N)); "aucpr": ap_q (the
    precision-recall kernels; AP = raw / 2^30 / P); "logloss": loss_q (gbdt_eval; log-loss = raw /
    2^30 / n).  Device rows: tree_perm.hip fills a margin buffer of at most ``max_bytes`` per group of
    columns, the metric kernels score the group's columns on the same stream into one int64 table,
    and the table is read back ONCE at the end; the grouping changes no result.  A feature no node
    splits on is not launched: its columns are the baseline.  CPU rows: the oracle margins scored by
    reference_gbdt.twice_pairs / ap_q / eval_record.  ValueError for an unknown scoring, a bad
    feature list, y of the wrong length and, for "auc" / "aucpr", a class without rows."""
    if scoring not in SCORINGS:
        raise ValueError(f"scoring must be one of {SCORINGS}, not {scoring!r}")
    ens = expl.ens
    _check_rows(X, expl)
    fs = R.perm_check(ens, features, n_repeats, seed)
    n, F, Rn = int(X.shape[0]), len(fs), int(n_repeats)
    if y.dim() != 1 or y.shape[0] != n or y.dtype != torch.uint8 or y.device != X.device:
        raise ValueError(f"y must be uint8 [{n}] on X's device")
    if n < 1:
        raise ValueError("permutation importance needs at least one row")
    if n > R.EVAL_MAX_ROWS:
        raise ValueError("at most 2^27 rows")

    def check_classes(P):
        if scoring != "logloss" and not 0 < P < n:
            raise ValueError(f'scoring "{scoring}" needs rows of both classes, y has {P} positives of {n}')

    if not X.is_cuda:
        yh = y.numpy()
        P = int(np.count_nonzero(yh))
        check_classes(P)
        pm, base = permuted_margins(X, expl, fs, Rn, seed)
        score = {"auc": R.twice_pairs, "aucpr": R.ap_q, "logloss": lambda m, yy: int(R.eval_record(m, yy)[0])}[scoring]
        raw = np.array([[score(pm[i, r], yh) for r in range(Rn)] for i in range(F)], np.int64).reshape(F, Rn)
        return raw, int(score(base, yh)), P
    from .scaler import scale_cast

    dev = X.device
    m = native()
    s = stream_of(X)
    t = _device_ensemble(expl, dev)
    used = feature_masks(ens).any(0)
    cols = [(-1, 0)] + [(f, r) for f in fs if used[f] for r in range(Rn)]      # column 0: the baseline
    tile = int(m.TREE_PERM_COLS)
    group = max(1, int(max_bytes) // (4 * n))
    group = min(len(cols), group // tile * tile if group >= tile else group)
    table = torch.zeros((len(cols), 4), dtype=torch.int64, device=dev)         # gbdt_eval adds into its record
    buf = torch.empty((group, n), dtype=torch.float32, device=dev)
    if scoring == "auc":
        ws = torch.empty(int(m.auc_radix_workspace_bytes(n)), dtype=torch.uint8, device=dev)
        fl = torch.empty(len(cols), dtype=torch.float64, device=dev)
    elif scoring == "aucpr":
        from .metrics import pr_workspace

        ws = pr_workspace(n, dev)
        fl = torch.empty(len(cols), dtype=torch.float64, device=dev)
    Xs = scale_cast(X, t["stats"], out_dtype="f32")
    for g0 in range(0, len(cols), group):
        part = cols[g0:g0 + group]
        _launch(Xs, t, ens, expl.d, part, seed, buf)
        for j in range(len(part)):
            sc, rec = ptr(buf) + 4 * n * j, ptr(table) + 32 * (g0 + j)
            if scoring == "auc":
                m.auc_radix(sc, ptr(y), n, ptr(ws), rec, ptr(fl) + 8 * (g0 + j), s)
            elif scoring == "aucpr":
                m.pr_curve(sc, ptr(y), n, ptr(ws), 0, 0, 0, rec, ptr(fl) + 8 * (g0 + j), s)
            else:
                m.gbdt_eval(sc, ptr(y), 0, n, rec, s)
    host = table.cpu().numpy()                                                 # the one read-back
    base_raw, P, rows = _raw_of_record(scoring, host[0])
    if rows != n:
        raise RuntimeError("permutation_scores: the metric kernels did not see every row")
    check_classes(P)
    raw = np.full((F, Rn), base_raw, np.int64)
    j = 1
    for i, f in enumerate(fs):
        if used[f]:
            raw[i] = host[j:j + Rn, 0]
            j += Rn
    return raw, base_raw, P
