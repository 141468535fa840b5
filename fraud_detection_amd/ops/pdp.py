"""Partial dependence and ICE curves of a tree ensemble's margin (csrc/kernels/tree_pd.hip): the
grid's override words, the device wrapper and the CPU path (the numpy oracle of
ops/reference_gbdt.py).

A row's directions in a tree are one 32-bit word (bit k: heap node k sends the row right).  Placing
feature f in cell c only changes the bits of the nodes that split on f: ``mask[t]`` has those nodes'
bits and ``words[t, c]`` the bits cell c sets there, so the row's word in cell c is
``(bits & ~mask[t]) | words[t, c]`` -- what the kernel evaluates per (row, tree, cell)."""
from __future__ import annotations

import numpy as np
import torch

from . import reference_gbdt as R
from .native import native, ptr, stream_of


def override_words(ens, f: int, reps: np.ndarray | None = None):
    """(mask uint32 [T], words uint32 [T, C]) of feature f over its cells (reference_gbdt.pd_cells):
    a node on f sends value cell c right iff !(r_c < thr[node]) and the missing cell right iff its
    default_left byte is 0."""
    if reps is None:
        reps, _ = R.pd_cells(ens, f)
    T, ni = ens.feat.shape
    missing = bool(len(reps)) and bool(np.isnan(reps[-1]))
    mask = np.zeros(T, np.uint32)
    words = np.zeros((T, len(reps)), np.uint32)
    for n in range(ni):
        on = ens.feat[:, n] == f
        if not on.any():
            continue
        bit = np.uint32(2 << n)
        right = ~(reps[None, :] < ens.thr[:, n].astype(np.float32)[:, None])
        if missing:
            right[:, -1] = ens.default_left[:, n] == 0
        mask |= np.where(on, bit, np.uint32(0))
        words |= np.where(on[:, None] & right, bit, np.uint32(0))
    return mask, words


def pd_design(ens, features):
    """(features, reps per feature, mask [T], word table per feature) -- what a launch needs."""
    fs, reps, _ = R.pd_check(ens, features, 0)
    mask = np.zeros(ens.n_trees, np.uint32)
    words = []
    for f, r in zip(fs, reps):
        m, w = override_words(ens, f, r)
        mask |= m
        words.append(w)
    return fs, reps, mask, words


def ice_from_words(Xs: np.ndarray, ens, features) -> np.ndarray:
    """float32 [n, C]: the kernel's formulation in numpy -- direction words once per (row, tree),
    overridden per cell, leaves added in tree order in fp32.  Equals partial_dependence_reference's
    ICE bit for bit; the CPU tests pin the override words with it."""
    from ..models.explainers import _margins_from_bits, path_direction_bits

    _, _, mask, words = pd_design(ens, features)
    W = words[0] if len(words) == 1 else (words[0][:, :, None] | words[1][:, None, :]).reshape(ens.n_trees, -1)
    bits = path_direction_bits(np.asarray(Xs, np.float32), ens) & ~mask[:, None]       # [T, n]
    return _margins_from_bits(bits[:, :, None] | W[:, None, :], ens)                    # [n, C]


def _device_design(expl, dev):
    """The explainer's ensemble and scaler on the device, cached on it per device; the override words
    of every feature set asked for so far are cached beside them."""
    key = str(dev)
    if expl._dev_cache is not None and expl._dev_cache[0] == key:
        return expl._dev_cache[1]
    from .scaler import stats_from_numpy

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)

    ens = expl.ens
    t = {"feat": up(ens.feat, np.int32), "thr": up(ens.thr, np.float32), "leaf": up(ens.leaf, np.float32),
         "dleft": up(ens.default_left, np.uint8) if ens.has_default_left else None,
         "stats": stats_from_numpy(expl.mean, expl.scale, device=dev), "words": {}}
    expl._dev_cache = (key, t)
    return t


def _device_words(t, ens, fs, dev):
    if fs not in t["words"]:
        _, reps, mask, words = pd_design(ens, fs)
        t["words"][fs] = (torch.from_numpy(mask.view(np.int32)).to(dev),
                          *(torch.from_numpy(np.ascontiguousarray(w).view(np.int32)).to(dev) for w in words))
    return t["words"][fs]


def partial_dependence(X: torch.Tensor, expl, features, ice: bool = False, sync: bool = True):
    """Brute partial dependence and, if ``ice``, the ICE curves of ``expl`` (a TreePartialDependence)
    over the RAW fp32 rows X [n, d] (unit column stride, any row stride; standardized with the
    explainer's scaler, a NaN stays NaN and follows default_left) -> (pd_q int64 [C], ice float32
    [n, C] or None), C the cells of the feature or, flattened ca * C_b + cb, of the pair.  Device
    rows run csrc/kernels/tree_pd.hip (numpy results if ``sync`` else device tensors); CPU rows run
    the oracle.  n = 0 gives zero sums."""
    ens = expl.ens
    if X.dim() != 2 or X.dtype != torch.float32 or X.shape[1] != expl.d or (X.shape[0] and X.stride(1) != 1):
        raise ValueError(f"X must be float32 [n, {expl.d}] with unit column stride")
    n = int(X.shape[0])
    fs, reps, _ = R.pd_check(ens, features, n)
    if not X.is_cuda:
        from ..models.explainers import _standardize

        q, ic = R.partial_dependence_reference(_standardize(X.numpy(), expl.mean, expl.scale), ens, fs, ice)
        return (q, ic) if sync else (torch.from_numpy(q), None if ic is None else torch.from_numpy(ic))
    from .scaler import scale_cast

    dev = X.device
    t = _device_design(expl, dev)
    mask, wa, *wb = _device_words(t, ens, fs, dev)
    ca, cb = len(reps[0]), (len(reps[1]) if len(fs) == 2 else 1)
    pd_q = torch.empty(ca * cb, dtype=torch.int64, device=dev)
    out = torch.empty((n, ca * cb), dtype=torch.float32, device=dev) if ice else None
    Xs = scale_cast(X, t["stats"], out_dtype="f32") if n else None
    native().tree_pd(ptr(Xs), n, Xs.stride(0) if n else expl.d, expl.d, ptr(t["feat"]), ptr(t["thr"]),
                     ptr(t["leaf"]), ptr(t["dleft"]), ptr(mask), ptr(wa), ca, ptr(wb[0]) if wb else 0, cb,
                     ens.n_trees, ens.depth, float(ens.base_margin), ptr(pd_q), ptr(out), stream_of(X))
    if not sync:
        return pd_q, out
    return pd_q.cpu().numpy(), None if out is None else out.cpu().numpy()
