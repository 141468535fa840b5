"""K8 k-nearest neighbours (SMOTE) and K9 SMOTE sample generation."""
from __future__ import annotations

import os

import numpy as np
import torch

from . import reference as ref
from .layout import DEFAULT_FP8_SCALE, DTYPE_KIND, NCOLS, check_rows, storage_kind
from .native import native, ptr, stream_of


def _pad32(n: int) -> int:
    return max(32, (n + 31) // 32 * 32)


def _padded(X: torch.Tensor, n_pad: int) -> torch.Tensor:
    if X.shape[0] == n_pad and X.is_contiguous():
        return X
    out = torch.zeros((n_pad, NCOLS), device=X.device, dtype=torch.float32)
    out[: X.shape[0]] = X
    return out


# Engines (all return the exact fp32 ranking, tests/test_kernels_gpu.py):
#   fp32    one-wave workgroups (32 queries) streaming candidate tiles from L2 / Infinity Cache
#           through a 16 x v_mfma_f32_32x32x2_f32 chain per 32x32 tile, the top-k kept in registers
#           -- knn.hip knn_topk_kernel.  auto: below 8k candidates.
#   bf16x3r every prepped row split x = hi + lo (two bf16 rows); the tile score hi.hi + hi.lo + lo.hi
#           (6 x v_mfma_f32_32x32x16_bf16: 5.3x fewer MFMA cycles) only filters, with no fp32 work in
#           the tile loop: passing candidates are appended to per-lane lists under a provable
#           lower-bound running threshold, and a second kernel re-scores the listed candidates exactly
#           (8 lanes per query) -- knn.hip knn_collect_kernel / knn_rerank_kernel.  auto: from 8k
#           candidates, wherever bf16x3t is not picked.  profiles/r5_k, r5_o: at the DP=8 global-scope
#           rank (13.6k queries x 108.8k candidates) 0.78 ms against fp32's 1.07; profiles/r6_knn: with
#           the quad-max pre-test in the append path and the pair-interleaved MFMA chains 0.184 ms
#           against fp32's 0.217 at the DP=1 self-search (13.6k x 13.6k), and in the pipeline's step
#           (quick SGD benches, two runs each) 1.006 / 1.015 ms medians against 1.037 / 1.035.
#   bf16x3t bf16x3r's score in TWO passes with a threshold that never moves: pass 1 keeps the maximum
#           of each of the 32 candidate groups c mod 32 per query, T = the K-th largest group maximum
#           minus the largest margin, pass 2 lists what can reach T (~5.6 candidates per query instead
#           of ~133) and a 32-lanes-per-query re-rank scores them exactly -- knn.hip
#           knn_groupmax_kernel / knn_threshold_kernel / knn_filter_kernel / knn_rerank_sparse_kernel.
#           auto: 8k..16k candidates with at least 4k queries, the one range it measured faster
#           (nothing between 13.6k and 108.8k candidates, or with fewer queries, has been measured).
#           profiles/pr4_knn_twopass: at the DP=1 self-search the lab has it at 0.128 ms against
#           bf16x3r's 0.160 (whole call, prep included) and the plain bench's step loses 24 us; at the
#           DP=8 global-scope rank it LOSES, 0.58 against 0.49 ms: there both passes stream the
#           candidates at ~45 % of the MFMA rate and the second pass costs more than bf16x3r's list
#           bookkeeping.
#   bf16x3f bf16x3t in ONE launch: a workgroup of W waves owns a pair of query blocks, wave y streams
#           tile slice y in both passes, and the group maxima, the threshold and the per-query lists
#           stay in LDS (no gmax / thr / lists / counts workspace); 16 lanes per query re-score the
#           listed candidates -- knn.hip knn_twopass_fused_kernel.  idx and score are bf16x3t's bit for
#           bit for every W.  nsplit= means W (at most KNN3F_MAX_WAVES: more is clamped, the result
#           does not depend on it).  bf16x3t stays as the staged form the stage tests read.
#           auto: where bf16x3t was picked (KNN_TWOPASS_ENGINE).  profiles/pr5_knn_fused: the lab's
#           DP=1 self-search 0.104 ms against bf16x3t's 0.126 and bf16x3r's 0.161 (whole call); the plain
#           bench's step, alternating with the parent, medians 0.873 / 0.869 / 0.861 ms against 0.893 /
#           0.900 / 0.895.  At the DP=8 rank it is bf16x3t's 0.58 ms against bf16x3r's 0.49: auto keeps
#           bf16x3r there.
# FDX_KNN (or engine=) selects one of the four.
# Retired, each measured slower than what replaced it: fp32lds (LDS-staged candidate chunks shared by
# 4-wave workgroups) and bf16x3 (the filter with an exact re-score inside the tile loop), 0.66-0.99x
# and 0.86-0.96x of fp32 from 13.6k to 170k rows (profiles/r2_s3i), bf16x3 superseded by bf16x3r
# (profiles/r5_k, r5_o); b3top (register top-8 approximate lists and a proof of exactness), 0.97 ms
# against bf16x3r's 0.79 at the DP=8 rank (profiles/r6_knn).  profiles/pr4_knn_twopass settled the
# set that stayed.
KNN_BF16X3_MIN_CANDIDATES = 1 << 13
KNN_TWOPASS_MAX_CANDIDATES = 1 << 14
KNN_TWOPASS_MIN_QUERIES = 1 << 12
KNN_TWOPASS_ENGINE = "bf16x3f"  # what auto runs in the two-pass range: bf16x3t or its one-launch form
KNN_ENGINES = ("fp32", "bf16x3r", "bf16x3t", "bf16x3f")


def knn_engine(mq: int, mc: int, engine: str | None = None) -> str:
    e = engine or os.environ.get("FDX_KNN", "auto")
    if e == "auto":
        if mc < KNN_BF16X3_MIN_CANDIDATES:
            return "fp32"
        return KNN_TWOPASS_ENGINE if mc <= KNN_TWOPASS_MAX_CANDIDATES and mq >= KNN_TWOPASS_MIN_QUERIES else "bf16x3r"
    if e not in KNN_ENGINES:
        raise ValueError(f"unknown k-NN engine {e!r}")
    return e


def _check_parents(parents: torch.Tensor | None, C: torch.Tensor, affine: torch.Tensor | None) -> int:
    if parents is None:
        if affine is not None:
            raise ValueError("parents_affine without parents")
        return 0
    if parents.dtype != torch.bfloat16 or tuple(parents.shape) != (C.shape[0], NCOLS) or \
            not parents.is_contiguous() or parents.device != C.device:
        raise ValueError("parents must be a contiguous bf16 [mc, 32] tensor on C's device")
    if affine is not None and (affine.dtype != torch.float64 or affine.numel() < 64 or affine.device != C.device):
        raise ValueError("parents_affine must be ScalerStats.aff (float64 [64]) on C's device")
    return ptr(parents)


def knn_topk(Q: torch.Tensor, C: torch.Tensor, k: int = 5, self_offset: int = -1, want_dist: bool = False,
             nsplit: int | None = None, engine: str | None = None, parents: torch.Tensor | None = None,
             parents_affine: torch.Tensor | None = None, _diag: dict | None = None, raw_stats=None,
             _operands: dict | None = None, list_cap: int | None = None):
    """k nearest candidates (squared L2 over the 30 feature columns) of each query row.

    Q [mq, 32] / C [mc, 32] fp32 padded rows (columns 30/31, intercept and label, are ignored).  If ``self_offset >= 0``, query row q is candidate
    row ``self_offset + q`` and is excluded (SMOTE's self-match removal).  Returns int32 [mq, k]
    (ascending distance, ties -> smaller index) and optionally squared distances.
    ``nsplit``: candidate slices searched by separate workgroups and merged (None = auto); for
    "bf16x3f" the waves W of a workgroup, each with its own slice.  ``list_cap`` ("bf16x3f" only): LDS
    list entries per query (None = KNN3F_LIST_CAP).
    ``engine``: "fp32" = exact fp32 MFMA chain over every candidate (16 x 32x32x2 f32 per tile);
    "bf16x3r" / "bf16x3t" / "bf16x3f" = a hi.hi + hi.lo + lo.hi bf16 MFMA filter (6 x 32x32x16 bf16 per tile)
    with a provable margin, the survivors listed under a running or a fixed threshold and re-scored
    exactly in fp32 by a second kernel (see the engine notes above); None/"auto" (FDX_KNN env) picks
    by size.  All return the exact fp32 ranking.
    ``parents`` (bf16 [mc, 32], optional): also filled with ``smote_parents(C, parents_affine)``
    by the operand-prep launch that already reads C (one launch fewer on the SMOTE path).
    ``raw_stats`` (``ScalerStats``; device self-search only, ``Q is C``): the rows are RAW padded
    minority rows (the fused scaler pass's ``MinorityRows.xraw[:count]``) and the prep launch
    standardizes them itself, z = (x - mean32) * inv32, bit for bit what ``scale_cast(...,
    out_dtype="f32", idx=...)`` wrote; ``parents`` are mapped through ``raw_stats.aff``
    (``parents_affine`` must be None).  Stats whose finalize is still owed
    (``scaler_fit_cast(defer_finalize=True)``) are finalized inside the same launch.
    """
    for t, nm in ((Q, "Q"), (C, "C")):
        if t.dim() != 2 or t.shape[1] != NCOLS or t.dtype != torch.float32:
            raise ValueError(f"{nm} must be fp32 [m, 32]")
    mq, mc = Q.shape[0], C.shape[0]
    if not 1 <= k <= 8:
        raise ValueError("k must be in [1, 8]")
    n_valid = mc - (1 if self_offset >= 0 else 0)
    if n_valid < k:
        raise ValueError(f"need at least k={k} candidates besides self, have {n_valid}")
    if self_offset >= 0 and self_offset + mq > mc:
        raise ValueError("self_offset + mq exceeds the candidate set")
    if raw_stats is not None:
        if not Q.is_cuda or Q.data_ptr() != C.data_ptr() or mq != mc or not Q.is_contiguous() \
                or not C.is_contiguous() or want_dist or parents_affine is not None or raw_stats.aff is None \
                or self_offset != 0:
            raise ValueError("raw_stats: a device self-search (Q is C, self_offset 0) over contiguous raw rows, "
                             "stats with aff, no parents_affine, no distances")
    if not Q.is_cuda:
        if _check_parents(parents, C, parents_affine):
            parents.copy_(smote_parents(C, parents_affine))
        idx, d2 = ref.knn_topk(Q.numpy(), C.numpy(), k, self_offset)
        idx_t = torch.from_numpy(idx)
        return (idx_t, torch.from_numpy(d2.astype(np.float32))) if want_dist else idx_t
    m = native()
    s = stream_of(Q)
    eng = knn_engine(mq, mc, engine)
    if list_cap is not None and eng != "bf16x3f":
        raise ValueError("list_cap is bf16x3f's")
    bf16 = eng != "fp32"  # bf16x3r / bf16x3t / bf16x3f: the filter streams hi/lo bf16 candidate tiles
    mq_pad, mc_pad = _pad32(mq), _pad32(mc)
    Qc, Cc = Q.contiguous(), C.contiguous()
    # GEMM-ready rows: the -0.5||c||^2 term rides in column 30 (see knn.hip knn_prep_kernel)
    Qp = torch.empty((mq_pad, NCOLS), device=Q.device, dtype=torch.float32)
    Cp = torch.empty((mc_pad, NCOLS), device=C.device, dtype=torch.float32)
    pp = _check_parents(parents, Cc, parents_affine)
    hl = (0, 0, 0)
    if bf16:  # the hi/lo bf16 operands (candidates in fragment order) + per-tile candidate norm bound
        Qhl = torch.empty((mq_pad, 64), device=Q.device, dtype=torch.bfloat16)
        Chl = torch.empty((mc_pad, 64), device=C.device, dtype=torch.bfloat16)
        tmax = torch.empty(mc_pad // 32, device=C.device, dtype=torch.float32)
        hl = (ptr(Chl), ptr(Qhl), ptr(tmax))
    if Qc.data_ptr() == Cc.data_ptr() and mq == mc:
        # SMOTE self-search: one launch reads the rows once and writes both operands (+ parents, and
        # for the bf16x3 engines their hi/lo split)
        if raw_stats is not None:
            st = raw_stats
            f = st.take_pending()  # the finalize still owed: folded into this launch
            if f is None:
                f = {"sums": None, "n": 0.0, "pivot": None, "colscale": None, "nparts": 0}
            m.knn_prep_raw(ptr(Cc), mc, mc_pad, ptr(Cp), ptr(Qp), pp, s, st.d, f["nparts"], f["n"], ptr(f["sums"]),
                           ptr(f["pivot"]), ptr(f["colscale"]), ptr(st.mean64), ptr(st.var64), ptr(st.scale64),
                           ptr(st.mean32), ptr(st.inv32), ptr(st.aff), *hl)
        else:
            m.knn_prep(ptr(Cc), mc, mc_pad, 2, ptr(Cp), s, ptr(Qp), ptr(parents_affine), pp, *hl)
    else:
        m.knn_prep(ptr(Cc), mc, mc_pad, 0, ptr(Cp), s, 0, ptr(parents_affine), pp)
        m.knn_prep(ptr(Qc), mq, mq_pad, 1, ptr(Qp), s)
        if bf16:  # the split the fused prep did not write: role 2 = candidates, 1 = queries
            m.knn_split(ptr(Cp), mc_pad, 2, ptr(Chl), ptr(tmax), s)
            m.knn_split(ptr(Qp), mq_pad, 1, ptr(Qhl), 0, s)
    if _operands is not None:  # the prep launch's outputs (tests)
        _operands.update(Cp=Cp, Qp=Qp)
        if bf16:
            _operands.update(Chl=Chl, Qhl=Qhl, tmax=tmax)
    idx = torch.empty((mq, k), device=Q.device, dtype=torch.int32)
    score = torch.empty((mq, k), device=Q.device, dtype=torch.float32) if want_dist else None
    if nsplit is not None:
        ns = max(1, int(nsplit))
    else:
        ns = {"fp32": m.knn_splits, "bf16x3r": m.knn3r_splits, "bf16x3t": m.knn3t_splits,
              "bf16x3f": m.knn3f_waves}[eng](mq_pad, mc_pad)
    if eng == "fp32":
        ws_s = ws_i = None
        if ns > 1:  # the slices' lists, merged by a second kernel
            ws_s = torch.empty((ns, mq, k), device=Q.device, dtype=torch.float32)
            ws_i = torch.empty((ns, mq, k), device=Q.device, dtype=torch.int32)
        m.knn_topk(ptr(Qp), mq_pad, mq, ptr(Cp), mc_pad, mc, int(self_offset), int(k), ptr(idx),
                   ptr(score), ptr(ws_s), ptr(ws_i), ns, s)
    elif eng == "bf16x3f":
        ns = min(ns, int(m.KNN3F_MAX_WAVES))
        cap = int(m.KNN3F_LIST_CAP) if list_cap is None else int(list_cap)
        scanned = torch.empty(mq, device=Q.device, dtype=torch.uint8) if _diag is not None else None
        m.knn_topk3f(ptr(Qp), ptr(Qhl), mq_pad, mq, ptr(Cp), ptr(Chl), ptr(tmax), mc_pad, mc, int(self_offset),
                     int(k), ptr(idx), ptr(score), ptr(scanned), ns, cap, s)
        if _diag is not None:  # which queries took the exact scan (diagnostics; synchronises)
            _diag.update(nsplit=ns, list_cap=cap, exact_scans=int(scanned.sum()), scanned=scanned.bool())
    else:
        qb = mq_pad // 32
        nb = ns * qb * 64
        lists = torch.empty(nb * m.KNN3R_LIST_CAP * 2, device=Q.device, dtype=torch.int32)  # (lb, index)
        # list lengths, then each lane's threshold and largest margin (knn_collect_kernel: its final
        # running threshold; knn_filter_kernel: the query's fixed T)
        counts = torch.empty(3 * nb, device=Q.device, dtype=torch.int32)
        if eng == "bf16x3r":
            m.knn_topk3r(ptr(Qp), ptr(Qhl), mq_pad, mq, ptr(Cp), ptr(Chl), ptr(tmax), mc_pad, mc, int(self_offset),
                         int(k), ptr(idx), ptr(score), ptr(lists), ptr(counts), ns, s)
        else:
            gmax = torch.empty(ns * qb * 17 * 64, device=Q.device, dtype=torch.float32)  # pass 1's group maxima
            thr = torch.empty(2 * mq_pad, device=Q.device, dtype=torch.float32)          # T, then M, per query
            m.knn_topk3t(ptr(Qp), ptr(Qhl), mq_pad, mq, ptr(Cp), ptr(Chl), ptr(tmax), mc_pad, mc, int(self_offset),
                         int(k), ptr(idx), ptr(score), ptr(lists), ptr(counts), ptr(gmax), ptr(thr), ns, s)
            if _operands is not None:  # the stages' outputs (tests)
                _operands.update(gmax=gmax.view(ns, qb, 17, 64), thr=thr.view(2, mq_pad),
                                 lists=lists.view(ns, qb, m.KNN3R_LIST_CAP, 64, 2), counts=counts.view(3, ns, qb, 64))
        if _diag is not None:  # list lengths and exact scans (diagnostics; synchronises)
            cn = counts[:nb].view(ns, qb, 64)
            c = cn.float().flatten()
            over_q = (cn > m.KNN3R_LIST_CAP).view(ns, qb, 2, 32).any(2).any(0).flatten()[:mq]  # [query]
            _diag.update(nsplit=ns, list_cap=int(m.KNN3R_LIST_CAP), mean=float(c.mean()), max=int(c.max()),
                         p99=float(torch.quantile(c[: min(c.numel(), 1 << 24)], 0.99)),
                         over_cap=int((c > m.KNN3R_LIST_CAP).sum()), counts=cn,
                         per_query=float(c.sum()) / mq, exact_scans=int(over_q.sum()), scanned=over_q)
    if want_dist:
        if _operands is not None:  # the engine's own scores q.c - 0.5||c||^2 (tests)
            _operands.update(score=score)
        qn = (Q[:, :30].double() ** 2).sum(1, keepdim=True)
        return idx, (qn - 2.0 * score.double()).float()
    return idx


def smote_parents(C: torch.Tensor, affine: torch.Tensor | None = None) -> torch.Tensor:
    """bf16 [m, 32] SMOTE parents in the training rows' space: bf16(z * sigma + c) on the feature
    columns with ``affine`` (ScalerStats.aff, pivot-shifted rows), bf16(z) without; columns 30/31
    copied.  Sampling from them halves the gather bytes and drops the per-sample affine map."""
    if C.dtype != torch.float32 or C.dim() != 2 or C.shape[1] != NCOLS:
        raise ValueError("C must be fp32 [m, 32]")
    C = C.contiguous()
    if not C.is_cuda:
        v = C.numpy().copy()
        if affine is not None:
            a = affine.cpu().numpy()
            v[:, :30] = (v[:, :30] * (1.0 / a[32:62]).astype(np.float32)) + a[:30].astype(np.float32)
        return torch.from_numpy(v).to(torch.bfloat16)
    P = torch.empty((C.shape[0], NCOLS), dtype=torch.bfloat16, device=C.device)
    native().smote_parents(ptr(C), C.shape[0], ptr(affine), ptr(P), stream_of(C))
    return P


def smote_generate(C: torch.Tensor, nbr: torch.Tensor, q_offset: int, n_new: int, out: torch.Tensor,
                   seed: int = 42, counter_base: int = 0, label: float = 1.0,
                   fp8_scale: float = DEFAULT_FP8_SCALE, affine: torch.Tensor | None = None,
                   sample_offset: int = 0) -> torch.Tensor:
    """Write ``n_new`` synthetic rows into ``out`` (a [n_new, 32] bf16/fp32/fp8 view, e.g. the tail of
    the training buffer).  Sample s interpolates minority row (q_offset + i) toward neighbour
    nbr[i, kk] with Philox draws keyed by (seed, s, counter_base).  C: fp32 standardized parents,
    or bf16 parents from smote_parents (already in the output space; ``affine`` must be None).
    ``affine`` ([64] float64, ScalerStats.aff) with fp32 parents: ``out`` holds pivot-shifted rows
    -- each feature is written as z * sigma + c.  ``sample_offset`` (multiple of 128): these are
    samples [sample_offset, sample_offset + n_new) of one global draw sequence (DP ranks)."""
    if C.dtype not in (torch.float32, torch.bfloat16) or C.dim() != 2 or C.shape[1] != NCOLS:
        raise ValueError("C must be fp32 or bf16 [m, 32]")
    pb = C.dtype == torch.bfloat16
    if pb and affine is not None:
        raise ValueError("bf16 parents are already in the output space (smote_parents): no affine")
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError("nbr must be int32 [mq, k]")
    mq, k = nbr.shape
    if q_offset < 0 or q_offset + mq > C.shape[0]:
        raise ValueError("query rows out of range of C")
    ref.smote_check_ranges(C.shape[0], mq, k)
    if sample_offset < 0 or sample_offset % 128:
        raise ValueError("sample_offset must be a non-negative multiple of 128")
    check_rows(out, "out")
    if out.shape[0] != n_new:
        raise ValueError("out must have n_new rows")
    kind = storage_kind(out)
    if n_new == 0:
        return out
    if not C.is_cuda:
        nb = nbr.numpy()
        if nb.min() < 0 or nb.max() >= C.shape[0]:
            raise ValueError("neighbour index out of range")
        rows = ref.smote_generate(C.float().numpy(), nb, q_offset, n_new, seed, counter_base, label,
                                  sample_offset=sample_offset)
        if affine is not None:
            a = affine.cpu().numpy()
            sig = (1.0 / a[32:62]).astype(np.float32)
            rows[:, :30] = rows[:, :30] * sig + a[:30].astype(np.float32)
        if kind == "bf16":
            out.copy_(torch.from_numpy(rows).to(torch.bfloat16))
        elif kind == "f32":
            out.copy_(torch.from_numpy(rows))
        else:
            r2 = rows.copy()
            r2[:, :30] *= fp8_scale
            out.copy_(torch.from_numpy(ref.fp8_encode(r2)))
        return out
    m = native()
    m.smote_generate(ptr(C), int(pb), ptr(nbr), mq, k, int(q_offset), int(n_new), int(sample_offset),
                     int(seed) & (2**64 - 1),
                     int(counter_base) & (2**64 - 1), float(label), DTYPE_KIND[kind], float(fp8_scale),
                     ptr(affine), ptr(out), stream_of(C))
    return out
