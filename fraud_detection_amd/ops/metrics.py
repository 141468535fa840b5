"""K10 exact ROC-AUC, confusion counts, and the exact precision-recall curve / average precision
with its operating points."""
from __future__ import annotations

import numpy as np
import torch

from . import reference as ref
from .native import native, ptr, stream_of

_CHUNK = 16384
# above this many positives the sorted-positive-chunk count (~N log(chunk) per 16384 positives)
# loses to the native radix sort + one counting pass
SORT_PATH_POSITIVES = 100_000
# from this many scores on, the radix path runs straight away (no positive-count read-back)
RADIX_ROWS = 8_000_000


def _radix_ws(dev, nbytes: int) -> torch.Tensor:
    """Sort scratch from the caching allocator, per call: its block is stream-ordered, so two AUC
    calls on different streams or threads never share keys / labels / counters (a module-level
    buffer reused by every call raced between concurrent evaluations -- ADVICE r3)."""
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def auc_radix(scores: torch.Tensor, labels: torch.Tensor):
    """Exact AUC on device with no host synchronisation: native stable LSD radix sort of
    (score key, label) + one counting pass (csrc/kernels/auc.hip).  Returns (auc float64 0-dim
    device tensor, int64 [3] device tensor = (twice_pairs, P, N))."""
    _check(scores, labels)
    n = scores.shape[0]
    m = native()
    dev = scores.device
    ws = _radix_ws(dev, int(m.auc_radix_workspace_bytes(n)))
    res = torch.empty(3, dtype=torch.int64, device=dev)
    auc = torch.empty((), dtype=torch.float64, device=dev)
    m.auc_radix(ptr(scores), ptr(labels), n, ptr(ws), ptr(res), ptr(auc), stream_of(scores))
    return auc, res


def auc_known_positives(scores: torch.Tensor, labels: torch.Tensor, n_pos: int):
    """Exact AUC on device with no host synchronisation when the caller knows the positive count
    (e.g. a CV fold, whose class counts the fold assignment already produced): the positives are
    compacted and chunk-sorted in LDS and every score counts the positives below it by binary search
    (~N log P) -- a handful of kernels instead of the 5-pass radix sort.  Returns (auc float64 0-dim
    device tensor, twice_pairs int64 0-dim device tensor)."""
    _check(scores, labels)
    n = scores.shape[0]
    P = int(n_pos)
    N = n - P
    dev = scores.device
    if P <= 0 or N <= 0:
        return torch.full((), float("nan"), dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
    if P > SORT_PATH_POSITIVES:
        auc, res = auc_radix(scores, labels)
        return auc, res[0]
    m = native()
    s = stream_of(scores)
    counter = torch.zeros(1, device=dev, dtype=torch.int64)
    pos = torch.empty(max(n, 1), device=dev, dtype=torch.float32)
    m.auc_compact(ptr(scores), ptr(labels), n, ptr(pos), ptr(counter), s)
    # the smallest power-of-two chunk that holds the positives: the one-block bitonic sort's
    # stages and the count's LDS fill scale with it (a fixed 16384 for ~3.4k fold positives cost
    # more than the radix path it replaced)
    chunk = min(_CHUNK, max(64, 1 << (P - 1).bit_length()))
    nchunks = (P + chunk - 1) // chunk
    m.sort_chunks(ptr(pos), n, ptr(counter), chunk, nchunks, s)
    out = torch.zeros(1, device=dev, dtype=torch.int64)
    m.auc_count(ptr(scores), ptr(labels), n, ptr(pos), ptr(counter), chunk, nchunks, ptr(out), s)
    twice = out[0]
    return twice.double() / (2.0 * P * N), twice


def _check(scores: torch.Tensor, labels: torch.Tensor):
    if scores.dtype != torch.float32 or scores.dim() != 1:
        raise ValueError("scores must be 1-D float32")
    if labels.dtype != torch.uint8 or labels.shape != scores.shape:
        raise ValueError("labels must be uint8 aligned with scores")


def auc_pair_counts(scores: torch.Tensor, labels: torch.Tensor):
    """(twice_pairs, P, N): twice_pairs = 2 #{s_p > s_n} + #{s_p == s_n}.  Exact integers, so
    data-parallel shards combine by all-gathering positives (see parallel/dp.py)."""
    _check(scores, labels)
    n = scores.shape[0]
    if not scores.is_cuda:
        y = labels.numpy().astype(bool)
        P, N = int(y.sum()), int(n - y.sum())
        return ref.auc_twice_pairs(scores.numpy(), y), P, N  # the integer itself, not a rounded float
    if n >= RADIX_ROWS:
        _, res = auc_radix(scores, labels)
        twice, P, N = (int(v) for v in res.cpu())
        return twice, P, N
    m = native()
    s = stream_of(scores)
    counter = torch.zeros(1, device=scores.device, dtype=torch.int64)
    pos = torch.empty(max(n, 1), device=scores.device, dtype=torch.float32)
    m.auc_compact(ptr(scores), ptr(labels), n, ptr(pos), ptr(counter), s)
    P = int(counter.item())
    N = n - P
    if P == 0 or N == 0:
        return 0, P, N
    if min(P, N) > SORT_PATH_POSITIVES:
        _, res = auc_radix(scores, labels)
        return int(res[0].item()), P, N
    nchunks = (P + _CHUNK - 1) // _CHUNK
    m.sort_chunks(ptr(pos), n, ptr(counter), _CHUNK, nchunks, s)
    out = torch.zeros(1, device=scores.device, dtype=torch.int64)
    m.auc_count(ptr(scores), ptr(labels), n, ptr(pos), ptr(counter), _CHUNK, nchunks, ptr(out), s)
    return int(out.item()), P, N


def roc_auc(scores: torch.Tensor, labels: torch.Tensor) -> float:
    """Exact ROC-AUC (ties averaged), equal to sklearn.metrics.roc_auc_score.  Large inputs on a
    GPU take the sync-free radix path and read the result once."""
    if scores.is_cuda and scores.shape[0] >= RADIX_ROWS:
        _check(scores, labels)
        auc, _ = auc_radix(scores, labels)
        return float(auc.item())
    twice, P, N = auc_pair_counts(scores, labels)
    if P == 0 or N == 0:
        return float("nan")
    return twice / (2.0 * P * N)


def confusion_counts(scores: torch.Tensor, labels: torch.Tensor, threshold: float = 0.0) -> np.ndarray:
    """[tn, fp, fn, tp] with prediction = score > threshold (threshold 0 on logits == p > 0.5)."""
    _check(scores, labels)
    if not scores.is_cuda:
        return ref.confusion(scores.numpy(), labels.numpy(), threshold)
    m = native()
    out = torch.zeros(4, device=scores.device, dtype=torch.int64)
    m.confusion(ptr(scores), ptr(labels), scores.shape[0], float(threshold), ptr(out), stream_of(scores))
    return out.cpu().numpy()


# ---- exact precision-recall curve, average precision and operating points ---------------------
def pr_workspace(n: int, dev) -> torch.Tensor:
    """Workspace of the precision-recall kernels for up to ``n`` scores: a per-round caller (the
    GBDT's aucpr) allocates it once and passes it as ``ws``."""
    return torch.empty(int(native().pr_workspace_bytes(int(n))), dtype=torch.uint8, device=dev)


def _pr_ws(n: int, dev, ws):
    if ws is None:
        return _radix_ws(dev, int(native().pr_workspace_bytes(n)))
    if ws.dtype != torch.uint8 or ws.device != dev or ws.numel() < int(native().pr_workspace_bytes(n)):
        raise ValueError("ws must be a uint8 tensor of at least pr_workspace_bytes(n) on the scores' device")
    return ws


def average_precision_device(scores: torch.Tensor, labels: torch.Tensor, ws: torch.Tensor | None = None):
    """Exact average precision on device with no host synchronisation: the radix sort of
    (score key, label), a device-wide scan of (tie-group heads, positives), the tie-group walk and
    one integer reduction (csrc/kernels/auc.hip).  Returns (ap float64 0-dim device tensor,
    int64 [4] device tensor = (ap_q, P, N, G)) with ap = ap_q / 2^30 / P (NaN without positives),
    ap_q = sum over tie groups of rint(dtp * precision * 2^30): sklearn's average_precision_score
    within 2^-31, as an order-independent integer (ops/reference.py average_precision_q).  ``ws``:
    an optional caller-owned workspace (pr_workspace).  NaN scores are not supported, as in the AUC
    paths; +-inf are ordinary scores."""
    _check(scores, labels)
    n = scores.shape[0]
    dev = scores.device
    if n == 0:  # nothing to launch
        return (torch.full((), float("nan"), dtype=torch.float64, device=dev),
                torch.zeros(4, dtype=torch.int64, device=dev))
    m = native()
    ws = _pr_ws(n, dev, ws)
    res = torch.empty(4, dtype=torch.int64, device=dev)
    ap = torch.empty((), dtype=torch.float64, device=dev)
    m.pr_curve(ptr(scores), ptr(labels), n, ptr(ws), 0, 0, 0, ptr(res), ptr(ap), stream_of(scores))
    return ap, res


def average_precision(scores: torch.Tensor, labels: torch.Tensor) -> float:
    """Average precision (ties grouped), equal to sklearn.metrics.average_precision_score within
    2^-31; NaN without positives.  GPU tensors take the kernels, CPU tensors the numpy oracle.  NaN
    scores are not supported."""
    _check(scores, labels)
    if not scores.is_cuda:
        return ref.average_precision(scores.numpy(), labels.numpy())
    ap, _ = average_precision_device(scores, labels)
    return float(ap.item())


def pr_curve(scores: torch.Tensor, labels: torch.Tensor):
    """Exact precision-recall curve: (thr float32 [G], tp int64 [G], fp int64 [G]) numpy arrays
    over the G tie groups, descending threshold, tp / fp = positives / negatives with
    score >= thr[g] (precision_recall(...) turns them into sklearn's precision_recall_curve without
    its appended (1, 0) point).  On a GPU: the kernels of average_precision_device, one read-back
    of G and one of the three slices.  NaN scores are not supported; -0.0 and +0.0 are one group,
    reported as +0.0."""
    _check(scores, labels)
    n = scores.shape[0]
    if not scores.is_cuda or n == 0:
        return ref.pr_curve(scores.cpu().numpy(), labels.cpu().numpy())
    m = native()
    dev = scores.device
    ws = _pr_ws(n, dev, None)
    thr = torch.empty(n, dtype=torch.float32, device=dev)
    tp = torch.empty(n, dtype=torch.int32, device=dev)  # u32 counts
    fp = torch.empty(n, dtype=torch.int32, device=dev)
    res = torch.empty(4, dtype=torch.int64, device=dev)
    ap = torch.empty((), dtype=torch.float64, device=dev)
    m.pr_curve(ptr(scores), ptr(labels), n, ptr(ws), ptr(tp), ptr(fp), ptr(thr), ptr(res), ptr(ap), stream_of(scores))
    G = int(res[3].item())
    cnt = torch.stack([tp[:G], fp[:G]]).cpu().numpy().view(np.uint32).astype(np.int64)
    return thr[:G].cpu().numpy(), cnt[0], cnt[1]


def precision_recall(thr, tp, fp):
    """(precision, recall) float64 of a curve: tp / (tp + fp) and tp / P (NaN without positives)."""
    tp = np.asarray(tp, dtype=np.float64)
    fp = np.asarray(fp, dtype=np.float64)
    P = tp[-1] if tp.shape[0] else 0.0
    with np.errstate(all="ignore"):
        return tp / (tp + fp), (tp / P if P > 0 else np.full(tp.shape, np.nan))


def operating_point(thr, tp, fp, *, min_precision: float | None = None, min_recall: float | None = None,
                    max_alerts: int | None = None) -> dict:
    """The threshold of a curve (pr_curve / pr_curve_hist) that meets exactly one criterion, with
    prediction = ``score >= threshold`` (confusion_counts predicts with ``>``):

    ``min_precision``: the lowest threshold whose precision is >= the target (maximum recall);
    ``min_recall``: the highest threshold whose recall is >= the target;
    ``max_alerts``: the lowest threshold with tp + fp <= the budget.

    Returns threshold, tp, fp, precision, recall, alerts.  ValueError when no threshold qualifies
    or when none or several criteria are given."""
    given = [c is not None for c in (min_precision, min_recall, max_alerts)]
    if sum(given) != 1:
        raise ValueError("exactly one of min_precision, min_recall, max_alerts must be given")
    thr, tp, fp = np.asarray(thr), np.asarray(tp, dtype=np.int64), np.asarray(fp, dtype=np.int64)
    precision, recall = precision_recall(thr, tp, fp)
    if min_precision is not None:
        ok = np.flatnonzero(precision >= float(min_precision))
        pick = ok[-1] if ok.size else None
    elif min_recall is not None:
        ok = np.flatnonzero(recall >= float(min_recall))
        pick = ok[0] if ok.size else None
    else:
        ok = np.flatnonzero(tp + fp <= int(max_alerts))
        pick = ok[-1] if ok.size else None
    if pick is None:
        raise ValueError("no threshold of the curve meets the criterion")
    g = int(pick)
    return {"threshold": float(thr[g]), "tp": int(tp[g]), "fp": int(fp[g]), "precision": float(precision[g]),
            "recall": float(recall[g]), "alerts": int(tp[g] + fp[g])}


# ---- histogram AUC (K10 `auc_hist`): mergeable across ranks by summing histograms ------------
def _order_key_np(scores: np.ndarray) -> np.ndarray:
    return ref.order_key(scores)  # -0 == +0


def score_histogram(scores: torch.Tensor, labels: torch.Tensor, bits: int = 20) -> torch.Tensor:
    """int32 [2, 2^bits] counts of (negative, positive) scores per bin of the order-preserving key."""
    _check(scores, labels)
    nb = 1 << bits
    if not scores.is_cuda:
        key = _order_key_np(scores.numpy()) >> np.uint32(32 - bits)
        lab = labels.numpy() != 0
        h = np.stack([np.bincount(key[~lab], minlength=nb), np.bincount(key[lab], minlength=nb)]).astype(np.int32)
        return torch.from_numpy(h)
    hist = torch.zeros(2 * nb, dtype=torch.int32, device=scores.device)
    native().auc_hist(ptr(scores), ptr(labels), scores.shape[0], bits, ptr(hist), stream_of(scores))
    return hist.view(2, nb)


def auc_from_histogram(hist: torch.Tensor) -> tuple[int, int, int]:
    """(twice_pairs, P, N) with bins as tie classes: sum_b P_b (2 N_<b + N_b), exact integers."""
    nb = hist.shape[1]
    bits = nb.bit_length() - 1
    if not hist.is_cuda:
        h = hist.numpy().astype(np.int64)
        nbefore = np.concatenate([[0], np.cumsum(h[0])[:-1]])
        twice = int(np.sum(h[1] * (2 * nbefore + h[0])))
        return twice, int(h[1].sum()), int(h[0].sum())
    out = torch.zeros(3, dtype=torch.int64, device=hist.device)
    native().auc_hist_reduce(ptr(hist), bits, ptr(out), stream_of(hist))
    twice, P, N = (int(v) for v in out.cpu())
    return twice, P, N


def roc_auc_hist(scores: torch.Tensor, labels: torch.Tensor, bits: int = 20, comm=None) -> float:
    """ROC-AUC from score histograms (scores in one bin count as ties).  With ``comm`` the
    histograms of all ranks are summed (one fixed-size all-reduce, collective C6) instead of
    gathering every score; 2^20 bins resolve float32 scores to ~2^-11 relative."""
    hist = score_histogram(scores, labels, bits)
    if comm is not None and comm.world_size > 1:
        hist = comm.all_reduce_(hist.contiguous())
    twice, P, N = auc_from_histogram(hist)
    if P == 0 or N == 0:
        return float("nan")
    return twice / (2.0 * P * N)


def roc_curve_hist(scores: torch.Tensor, labels: torch.Tensor, bits: int = 16, comm=None):
    """(fpr, tpr) at every bin edge, descending threshold -- the evaluate_model.py ROC plot."""
    hist = score_histogram(scores, labels, bits)
    if comm is not None and comm.world_size > 1:
        hist = comm.all_reduce_(hist.contiguous())
    h = hist.cpu().numpy().astype(np.int64)[:, ::-1]
    tp, fp = np.cumsum(h[1]), np.cumsum(h[0])
    P, N = max(tp[-1], 1), max(fp[-1], 1)
    keep = np.r_[True, (np.diff(tp) + np.diff(fp)) > 0]
    return np.r_[0.0, fp[keep] / N], np.r_[0.0, tp[keep] / P]


def pr_curve_hist(scores: torch.Tensor, labels: torch.Tensor, bits: int = 16, comm=None):
    """(thr, tp, fp) as pr_curve, from score histograms with every non-empty bin as one tie group
    -- the data-parallel form: with ``comm`` the histograms of all ranks are summed (one fixed-size
    all-reduce) instead of gathering every score.  thr[g] is the bin's lower edge, the smallest
    score the bin can hold (so ``score >= thr[g]`` selects the bin and everything above it; -inf
    for the bin of -inf).  When all scores in a bin are equal, tp / fp equal the exact curve's, and
    so does thr for non-negative scores whose low 32 - bits mantissa bits are zero."""
    hist = score_histogram(scores, labels, bits)
    if comm is not None and comm.world_size > 1:
        hist = comm.all_reduce_(hist.contiguous())
    h = hist.cpu().numpy().astype(np.int64)
    nz = np.flatnonzero(h[0] + h[1])[::-1]  # non-empty bins, descending
    tp, fp = np.cumsum(h[1][nz]), np.cumsum(h[0][nz])
    with np.errstate(invalid="ignore"):
        thr = ref.order_key_inv(nz.astype(np.uint32) << np.uint32(32 - bits))
        thr = np.where(np.isnan(thr), np.float32(-np.inf), thr).astype(np.float32)
    return thr, tp.astype(np.int64), fp.astype(np.int64)


def average_precision_hist(scores: torch.Tensor, labels: torch.Tensor, bits: int = 16, comm=None) -> float:
    """Average precision of pr_curve_hist's curve (scores in one bin count as ties), by the exact
    curve's integer formula; NaN without positives.  The data-parallel answer, as roc_auc_hist is
    for the AUC."""
    _, tp, fp = pr_curve_hist(scores, labels, bits, comm)
    P = int(tp[-1]) if tp.shape[0] else 0
    return ref.ap_q_from_curve(tp, fp) / ref.AP_SCALE / P if P else float("nan")
