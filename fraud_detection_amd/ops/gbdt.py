"""K11 GBDT ops: quantile binning, boosting rounds and inference (csrc/kernels/gbdt.hip).

Device path: one boosting round = gradient kernel -> per level (histogram, [RCCL all-reduce of the
int64 histograms and child counts under DP], split, stable partition) -> leaf values -> margin
update.  Nothing in a round synchronises with the host.  CPU tensors run the numpy oracle
(ops/reference_gbdt.py), which builds the same trees from the same quantised gradients.
"""
from __future__ import annotations

import os
import warnings
from dataclasses import dataclass, field, replace

import numpy as np
import torch

from . import reference_gbdt as R
from .native import native, ptr, stream_of

MAX_BIN = R.MAX_BIN
MAX_FEAT = 30
HIST_ENTRIES = MAX_FEAT * MAX_BIN * 2
# partition grid (<= 4096): 2048 blocks of 256 -- count kernel 57.5 us vs 62.0 at 1024 per level at
# 16M rows, scatter unchanged; 4096 and 512 slower, and 8 rows per thread instead of 4 slowed both
# kernels (67-79 us) (profiles/r5_zp, r5_zq)
PART_BLOCKS = int(os.environ.get("FDX_GBDT_PART_BLOCKS", "2048"))


def normalize_monotone(mc):
    """xgboost's ``monotone_constraints`` in one of its forms -> None, a tuple of ints in {-1, 0, 1}
    (one per feature) or a dict {feature index: sign} with int keys >= 0.  Accepted: a sequence of
    ints, the string form "(1,0,-1)", a dict.  Anything else is a ValueError."""
    def sign(v):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or int(v) not in (-1, 0, 1):
            raise ValueError(f"monotone_constraints: every entry must be the integer -1, 0 or 1, got {v!r}")
        return int(v)

    if mc is None:
        return None
    if isinstance(mc, str):
        body = mc.strip()
        if body.startswith("(") and body.endswith(")"):
            body = body[1:-1]
        try:
            mc = [int(tok) for tok in body.split(",") if tok.strip()]
        except ValueError:
            raise ValueError(f"monotone_constraints: cannot parse {mc!r}; the string form is '(1,0,-1)'") from None
    if isinstance(mc, dict):
        out = {}
        for k, v in mc.items():
            if isinstance(k, str) and k.strip().lstrip("+-").isdigit():
                k = int(k)
            if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or int(k) < 0:
                raise ValueError(f"monotone_constraints: dict keys are feature indices >= 0, got {k!r} "
                                 "(feature names are resolved by the train entry point)")
            if int(k) in out:
                raise ValueError(f"monotone_constraints: feature {int(k)} is named twice")
            out[int(k)] = sign(v)
        return out
    if isinstance(mc, (list, tuple, np.ndarray)):
        return tuple(sign(v) for v in (mc.tolist() if isinstance(mc, np.ndarray) else mc))
    raise ValueError(f"monotone_constraints must be a sequence of ints, a string like '(1,0,-1)' or a dict, got {mc!r}")


MAX_GROUPS = 32  # interaction groups of one fit (the split kernel takes their masks by value)


def normalize_interaction(ic):
    """xgboost's ``interaction_constraints`` in one of its forms -> None or a tuple of groups, each a
    sorted tuple of feature indices >= 0; a group given twice is kept once, empty groups are dropped,
    and nothing left is None.  Accepted: a nested sequence of ints, the string form
    "[[0, 2], [1, 3, 4]]", None.  A non-integer, a bool, a negative index, a feature repeated inside
    one group or anything unparsable is a ValueError."""
    if ic is None:
        return None
    if isinstance(ic, str):
        import json

        try:
            ic = json.loads(ic)
        except ValueError:
            raise ValueError(f"interaction_constraints: cannot parse {ic!r}; the string form is "
                             "'[[0, 2], [1, 3, 4]]'") from None
    if isinstance(ic, np.ndarray):
        ic = ic.tolist()
    if not isinstance(ic, (list, tuple)):
        raise ValueError(f"interaction_constraints must be a list of lists of feature indices, a string like "
                         f"'[[0, 2], [1, 3, 4]]' or None, got {ic!r}")
    out = []
    for g in ic:
        if isinstance(g, np.ndarray):
            g = g.tolist()
        if not isinstance(g, (list, tuple)):
            raise ValueError(f"interaction_constraints: every group must be a list of feature indices, got {g!r}")
        for v in g:
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or int(v) < 0:
                raise ValueError(f"interaction_constraints: feature indices are integers >= 0, got {v!r} "
                                 "(feature names are resolved by the train entry point)")
        grp = tuple(sorted(int(v) for v in g))
        if len(set(grp)) != len(grp):
            raise ValueError(f"interaction_constraints: a feature is repeated inside the group {list(g)!r}")
        if grp and grp not in out:
            out.append(grp)
    return tuple(out) or None


@dataclass
class GBDTParams:
    """xgboost.XGBClassifier parameter names and defaults used by train_model.py:69-80."""
    n_estimators: int = 100
    learning_rate: float = 0.1
    max_depth: int = 5
    reg_lambda: float = 1.0
    min_child_weight: float = 1.0
    gamma: float = 0.0
    max_bin: int = 256
    scale_pos_weight: float = 1.0
    base_score: float = 0.5
    cut_sample_rows: int = 1 << 20
    # stochastic boosting: stateless Philox draws of (seed, round, global row | feature),
    # reference_gbdt.row_sample_mask / feature_masks.  With every fraction at 1.0 the seed has no
    # effect and the fit is the deterministic full-data fit, launch for launch.
    subsample: float = 1.0
    colsample_bytree: float = 1.0
    colsample_bylevel: float = 1.0
    colsample_bynode: float = 1.0
    seed: int = 0
    # "last_bin": a NaN is binned with the feature's largest values and always goes right.
    # "learn": NaN gets a bin slot of its own and every split learns which side it goes to
    # (xgboost's sparsity-aware split finding; reference_gbdt's module docstring has the rules).
    missing_policy: str = "last_bin"
    # xgboost's monotone_constraints: per feature +1 (the score never falls as the feature rises), -1
    # (never rises) or 0.  A sequence of d ints, the string "(1,0,-1)" or {feature index: sign};
    # None or all zero: unconstrained, launch for launch (fit_binned has the rules).
    monotone_constraints: tuple | dict | str | None = None
    # xgboost's interaction_constraints: groups of feature indices.  Below a path of split features
    # a node may use the path's own features and every group that contains the whole path
    # (reference_gbdt's module docstring has the rule).  A nested sequence of ints or the string
    # "[[0, 2], [1, 3, 4]]"; None or no non-empty group: unconstrained, launch for launch.
    interaction_constraints: tuple | list | str | None = None
    # xgboost's reg_alpha (L1 on the leaf weights: the soft threshold of G in weight and gain) and
    # max_delta_step (|weight| capped before the monotone clamp; 0 = no cap, the knob xgboost
    # recommends for logistic loss on extremely imbalanced classes).  Both finite and >= 0; both 0:
    # the fit without them, launch for launch (fit_binned has the rules).
    reg_alpha: float = 0.0
    max_delta_step: float = 0.0

    MISSING_POLICIES = ("last_bin", "learn")
    # fields a checkpoint signature names only off their defaults (older checkpoints resume): the
    # sampling fields and, added the same way, the missing policy
    SAMPLING_DEFAULTS = {"subsample": 1.0, "colsample_bytree": 1.0, "colsample_bylevel": 1.0,
                         "colsample_bynode": 1.0, "seed": 0, "missing_policy": "last_bin",
                         "monotone_constraints": None, "interaction_constraints": None,
                         "reg_alpha": 0.0, "max_delta_step": 0.0}

    @property
    def colsampled(self) -> bool:
        return not (self.colsample_bytree == 1.0 and self.colsample_bylevel == 1.0 and self.colsample_bynode == 1.0)

    @property
    def sampled(self) -> bool:
        return self.subsample != 1.0 or self.colsampled

    @property
    def learn_missing(self) -> bool:
        return self.missing_policy == "learn"

    @property
    def reg(self):
        """(reg_alpha, max_delta_step) as floats, or None when both are 0 (nothing changes)."""
        a, m = float(self.reg_alpha), float(self.max_delta_step)
        return (a, m) if (a != 0.0 or m != 0.0) else None

    def monotone_signs(self, d: int):
        """int64 [d] signs of a d-feature fit, or None when nothing is constrained."""
        mc = normalize_monotone(self.monotone_constraints)
        if mc is None:
            return None
        if isinstance(mc, dict):
            bad = [k for k in mc if k >= d]
            if bad:
                raise ValueError(f"monotone_constraints: feature index {bad[0]} is out of range for {d} features")
            mc = tuple(mc.get(f, 0) for f in range(d))
        if len(mc) != d:
            raise ValueError(f"monotone_constraints has {len(mc)} entries, the fit has {d} features")
        return np.asarray(mc, np.int64) if any(mc) else None

    def interaction_masks(self, d: int):
        """The groups of a d-feature fit as a list of uint32 masks (bit f = feature f), or None when
        there is none."""
        ic = normalize_interaction(self.interaction_constraints)
        if ic is None:
            return None
        bad = [f for g in ic for f in g if f >= d]
        if bad:
            raise ValueError(f"interaction_constraints: feature index {bad[0]} is out of range for {d} features")
        if len(ic) > MAX_GROUPS:
            raise ValueError(f"interaction_constraints: {len(ic)} groups, at most {MAX_GROUPS} are supported")
        return [int(sum(1 << f for f in g)) for g in ic]

    def validate(self):
        self.monotone_constraints = normalize_monotone(self.monotone_constraints)
        self.interaction_constraints = normalize_interaction(self.interaction_constraints)
        if self.missing_policy not in self.MISSING_POLICIES:
            raise ValueError(f"missing_policy must be one of {self.MISSING_POLICIES}, got {self.missing_policy!r}")
        for name in ("subsample", "colsample_bytree", "colsample_bylevel", "colsample_bynode"):
            v = float(getattr(self, name))
            if not 0.0 < v <= 1.0:  # NaN fails too
                raise ValueError(f"{name} must be in (0, 1]")
        if isinstance(self.seed, bool) or not isinstance(self.seed, (int, np.integer)) or not 0 <= int(self.seed) < 1 << 64:
            raise ValueError("seed must be an integer in [0, 2^64)")
        if not 1 <= self.max_depth <= 7:
            raise ValueError("max_depth must be in [1, 7] (node ids are stored in one byte)")
        if not 2 <= self.max_bin <= MAX_BIN:
            raise ValueError("max_bin must be in [2, 256]")
        if not 0.0 < self.base_score < 1.0:
            raise ValueError("base_score must be in (0, 1)")
        if self.n_estimators < 0 or self.learning_rate <= 0:
            raise ValueError("bad n_estimators / learning_rate")
        for name in ("reg_lambda", "min_child_weight", "gamma", "reg_alpha", "max_delta_step"):
            v = float(getattr(self, name))
            if not np.isfinite(v) or v < 0.0:
                raise ValueError(f"{name} must be finite and >= 0")
        if not np.isfinite(float(self.scale_pos_weight)) or self.scale_pos_weight <= 0:
            raise ValueError("scale_pos_weight must be finite and > 0")
        return self


@dataclass
class TreeEnsemble:
    depth: int
    feat: np.ndarray   # [T, 2^D - 1] int32 (-1 = pass-through)
    bin: np.ndarray    # [T, 2^D - 1] int32
    thr: np.ndarray    # [T, 2^D - 1] float32
    gain: np.ndarray   # [T, 2^D - 1] float64
    leaf: np.ndarray   # [T, 2^D] float32
    cuts: np.ndarray   # [d, 256] float32
    nbins: np.ndarray  # [d] int32
    base_score: float = 0.5
    params: dict = field(default_factory=dict)
    default_left: np.ndarray | None = None  # [T, 2^D - 1] uint8: a NaN goes left at the node; None: all zero
    # [T, 2^(D+1)] float64 node covers by 1-based heap node (index 0 unused), node_cover's int64 sums
    # divided by 2^30 for cover_kind "hessian" (xgboost's sum_hess), the row counts themselves for
    # "count"; None: the model stores no cover (path-dependent TreeSHAP needs one)
    cover: np.ndarray | None = None
    cover_kind: str | None = None

    @property
    def has_default_left(self) -> bool:
        return self.default_left is not None and bool(np.any(self.default_left))

    def with_cover(self, q: np.ndarray, kind: str) -> "TreeEnsemble":
        """A copy of this ensemble that stores node_cover's int64 table ``q`` of ``kind``."""
        q = np.asarray(q)
        if q.shape != (self.n_trees, 2 << self.depth):
            raise ValueError(f"cover must be [{self.n_trees}, {2 << self.depth}], got {q.shape}")
        if kind not in R.COVER_KINDS:
            raise ValueError(f"cover kind must be one of {R.COVER_KINDS}, not {kind!r}")
        cover = q.astype(np.float64) / (R.COVER_SCALE if kind == "hessian" else 1.0)
        return replace(self, cover=cover, cover_kind=kind)

    def head(self, k: int) -> "TreeEnsemble":
        """The first k trees (and their covers)."""
        if not 1 <= k <= self.n_trees:
            raise ValueError(f"tree count must be in [1, {self.n_trees}]")
        if k == self.n_trees:
            return self
        cut = lambda a: None if a is None else a[:k]  # noqa: E731
        return replace(self, feat=self.feat[:k], bin=self.bin[:k], thr=self.thr[:k], gain=self.gain[:k],
                       leaf=self.leaf[:k], default_left=cut(self.default_left), cover=cut(self.cover))

    @property
    def n_trees(self) -> int:
        return int(self.feat.shape[0])

    @property
    def n_features(self) -> int:
        return int(self.nbins.shape[0])

    @property
    def base_margin(self) -> float:
        return float(np.log(self.base_score / (1.0 - self.base_score)))

    def feature_importance(self, kind: str = "gain") -> np.ndarray:
        """xgboost-style importances: "gain" (mean gain per split), "weight" (split count),
        "total_gain", and from the stored node covers "cover" (mean cover per split) and
        "total_cover"."""
        if kind not in ("gain", "weight", "total_gain", "cover", "total_cover"):
            raise ValueError(f"unknown importance kind {kind!r}")
        d = self.n_features
        cnt = np.zeros(d)
        tot = np.zeros(d)
        m = self.feat >= 0
        np.add.at(cnt, self.feat[m], 1.0)
        if kind in ("cover", "total_cover"):
            if self.cover is None:
                raise ValueError(f'importance kind "{kind}" needs node covers: run node_cover '
                                 "(GBDTClassifier.compute_cover, or fit(..., record_cover=True)) first")
            np.add.at(tot, self.feat[m], self.cover[:, 1: self.feat.shape[1] + 1][m])
        else:
            np.add.at(tot, self.feat[m], self.gain[m])
        if kind == "weight":
            return cnt
        if kind in ("total_gain", "total_cover"):
            return tot
        return np.where(cnt > 0, tot / np.maximum(cnt, 1), 0.0)

    def to_dict(self) -> dict:
        o = {"format": "fdx-gbdt/1", "depth": self.depth, "base_score": self.base_score,
             "params": self.params, "feat": self.feat.tolist(), "bin": self.bin.tolist(),
             "thr": [[float(v) if np.isfinite(v) else ("-inf" if v == -np.inf else "inf") for v in row] for row in self.thr],
             "gain": self.gain.tolist(), "leaf": self.leaf.tolist(),
             "cuts": [[float(v) if np.isfinite(v) else "inf" for v in row[:nb]] for row, nb in zip(self.cuts, self.nbins)],
             "nbins": self.nbins.tolist()}
        if self.has_default_left:  # an ensemble without a default-left node serialises as it always did
            o["default_left"] = np.asarray(self.default_left, np.uint8).tolist()
        if self.cover is not None:  # likewise: a model without cover writes the file it always wrote
            o["cover"] = np.asarray(self.cover, np.float64).tolist()
            o["cover_kind"] = self.cover_kind
        return o

    @classmethod
    def from_dict(cls, o: dict) -> "TreeEnsemble":
        if o.get("format") != "fdx-gbdt/1":
            raise ValueError("not an fdx-gbdt/1 model")
        f = lambda v: np.inf if v == "inf" else (-np.inf if v == "-inf" else float(v))  # noqa: E731
        depth = int(o["depth"])
        ni = (1 << depth) - 1
        nbins = np.asarray(o["nbins"], np.int32)
        cuts = np.full((len(nbins), MAX_BIN), np.inf, np.float32)
        for i, row in enumerate(o["cuts"]):
            cuts[i, : len(row)] = [f(v) for v in row]
        feat = np.asarray(o["feat"], np.int32).reshape(-1, ni)
        return cls(depth=depth, feat=feat, bin=np.asarray(o["bin"], np.int32).reshape(-1, ni),
                   thr=np.asarray([[f(v) for v in row] for row in o["thr"]], np.float32).reshape(-1, ni),
                   gain=np.asarray(o["gain"], np.float64).reshape(-1, ni),
                   leaf=np.asarray(o["leaf"], np.float32).reshape(-1, 1 << depth), cuts=cuts, nbins=nbins,
                   base_score=float(o["base_score"]), params=dict(o.get("params", {})),
                   default_left=(np.asarray(o["default_left"], np.uint8).reshape(-1, ni)
                                 if o.get("default_left") is not None else None),
                   cover=(np.asarray(o["cover"], np.float64).reshape(-1, 2 << depth)
                          if o.get("cover") is not None else None),
                   cover_kind=o.get("cover_kind") if o.get("cover") is not None else None)


# Device-side split words (csrc/kernels/gbdt.hip goes_right): a default-left split of bin b (b = -1:
# the missing rows alone go left) is 0x200 | (b + 1), a word in [0x200, 0x3ff]; every other word is
# the split bin itself, missing rows going right -- what the `bin` arrays always held.  With
# s = (w in [0x200, 0x3ff]) the walk on a bin byte v is right = ((v + s) & 0xff) > w - (s << 9):
# v > w for the old words; for the new ones byte 255 wraps to 0 and goes left, every other byte
# compares v + 1 > b + 1.
def encode_bin_words(binv: np.ndarray, default_left: np.ndarray | None) -> np.ndarray:
    binv = np.asarray(binv, np.int32)
    if default_left is None:
        return binv
    return np.where(np.asarray(default_left) != 0, 0x200 | (binv + 1), binv).astype(np.int32)


def decode_bin_words(words: np.ndarray):
    """(bin int32, default_left uint8) of device split words."""
    words = np.asarray(words, np.int32)
    dl = (words >> 9) == 1
    return np.where(dl, (words & 0x1FF) - 1, words).astype(np.int32), dl.astype(np.uint8)


# ---- binning ---------------------------------------------------------------------------------
def quantile_cuts(X: torch.Tensor, max_bin: int = MAX_BIN, sample_rows: int = 1 << 20, comm=None,
                  missing: bool = False):
    """Per-feature quantile cuts from a deterministic strided row sample.  Under DP every rank
    contributes a sample and the cuts come from the gathered sample, so all ranks agree.
    ``missing``: the quantiles of a feature are taken over the sample's non-NaN values only
    (reference_gbdt.quantile_cuts); at most 255 real bins, byte 255 being the missing slot."""
    n, d = X.shape
    if d > MAX_FEAT:
        raise ValueError(f"at most {MAX_FEAT} features")
    world = comm.world_size if comm is not None else 1
    per = max(1, sample_rows // world)
    stride = max(1, n // per)
    if comm is not None and world > 1:
        samp, _ = comm.all_gather_rows(X[::stride][:per].contiguous())
        src, m, step = samp, samp.shape[0], 1
    else:
        src, m, step = X, min(per, (n + stride - 1) // stride), stride
    if not src.is_cuda:
        return R.quantile_cuts(src[::step][:m].float().numpy(), max_bin, missing)
    # Exact order statistics by a native radix select (quantile.hip): the minimum and the max_bin - 1
    # quantile rows of the sample come back to the host, where deduplication is trivial.  Selection
    # is exact, so the cuts equal the CPU oracle's (np.sort) on the same sample.
    if src.dtype != torch.float32 or src.stride(1) != 1:
        src, step = src[::step][:m].float().contiguous(), 1
    nat = native()
    ws = torch.empty(nat.quantile_select_ws_bytes(m, d), dtype=torch.uint8, device=src.device)
    if missing:
        # the same select with per-feature rank bases m_f = the feature's non-NaN count, which stays
        # on the device; NaN sorts last, so a rank below m_f never lands on one, and a feature
        # without a value returns NaN as its minimum (cuts_from_sorted_picks: one bin)
        max_bin = min(max_bin, MAX_BIN - 1)
        samp = src[::step][:m]
        counts = (samp == samp).sum(0, dtype=torch.int64).contiguous()
    picks = torch.empty((max_bin, d), dtype=torch.float32, device=src.device)
    nat.quantile_select(ptr(src), m, step, src.stride(0), d, max_bin, ptr(ws), ptr(picks), stream_of(src),
                        *((ptr(counts),) if missing else ()))
    picks = picks.cpu().numpy()
    return R.cuts_from_sorted_picks(picks[1:], picks[0], max_bin, missing)


def bin_rows(X: torch.Tensor, cuts: np.ndarray, nbins: np.ndarray, out: torch.Tensor | None = None,
             missing: bool = False) -> torch.Tensor:
    """u8 [n, 32] bins (features in bytes 0..d-1).  ``out``: a [n, 32] u8 view to write (e.g. the
    SMOTE tail of a binned table).  ``missing``: a NaN goes to byte 255, the missing slot (the cuts
    then have at most 255 real bins), instead of the feature's last bin."""
    n, d = X.shape
    if out is not None and (tuple(out.shape) != (n, R.ROW_BYTES) or out.dtype != torch.uint8
                            or not out.is_contiguous() or out.device != X.device):
        raise ValueError("out must be a contiguous u8 [n, 32] tensor on X's device")
    if not X.is_cuda:
        b = torch.from_numpy(R.bin_rows(X.numpy(), cuts, nbins, missing))
        return out.copy_(b) if out is not None else b
    if X.dtype != torch.float32 or X.stride(1) != 1:
        raise ValueError("X must be float32 with unit column stride")
    m = native()
    out = out if out is not None else torch.empty((n, R.ROW_BYTES), dtype=torch.uint8, device=X.device)
    ct = torch.from_numpy(np.ascontiguousarray(cuts[:d])).to(X.device)
    nt = torch.from_numpy(np.ascontiguousarray(nbins[:d])).to(X.device)
    if missing and int(np.max(nbins[:d], initial=0)) > MAX_BIN - 1:
        raise ValueError("missing: byte 255 is the missing slot, at most 255 real bins per feature")
    if n:
        m.gbdt_bin(ptr(X), n, X.stride(0), d, ptr(ct), ptr(nt), ptr(out), stream_of(X), *((True,) if missing else ()))
    return out


# ---- training --------------------------------------------------------------------------------
# Rows a histogram block accumulates in LDS between flushes to its slot (0: the kernel's bound,
# 2^16 -- packed (h, g) words stay exact); tests lower it to exercise the multi-flush path.
HIST_FLUSH_ROWS = 0


class _Workspace:
    def __init__(self, n: int, depth: int, dev: torch.device):
        nheap = (2 << depth) - 1
        self.gh = torch.empty((n, 2), dtype=torch.int16, device=dev)  # (g, h) packed in 4 bytes
        self.ridx = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2)]
        self.nid = [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2)]
        self.flag = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        self.counts = torch.empty(PART_BLOCKS, dtype=torch.int64, device=dev)  # right rows per partition block
        self.seg = torch.zeros((nheap, 2), dtype=torch.int64, device=dev)
        self.node_r = torch.zeros(nheap, dtype=torch.int64, device=dev)  # right rows per node (zeroed per round)
        self.gcnt = torch.zeros(nheap, dtype=torch.int64, device=dev)
        self.hist = torch.zeros(((1 << depth) - 1) * HIST_ENTRIES, dtype=torch.int64, device=dev)
        # per-(node, block) histogram slots the histogram kernel writes without atomics
        self.slots = torch.empty(native().gbdt_hist_slot_words(), dtype=torch.int64, device=dev)
        self.ng = torch.zeros(nheap, dtype=torch.int64, device=dev)
        self.nh = torch.zeros(nheap, dtype=torch.int64, device=dev)
        # weight bounds per heap node of a monotone fit (gbdt_split writes them level by level)
        self.blo = torch.full((nheap,), -np.inf, dtype=torch.float64, device=dev)
        self.bhi = torch.full((nheap,), np.inf, dtype=torch.float64, device=dev)
        # split features of every heap node's ancestors, one bit each, of a fit with interaction
        # constraints (uint32 words; gbdt_split writes them level by level)
        self.path = torch.zeros(nheap, dtype=torch.int32, device=dev)


# ---- per-round evaluation and early stopping -------------------------------------------------
EVAL_METRICS = ("logloss", "error", "auc", "aucpr")


@dataclass
class EvalRecord:
    """What a fit with ``eval_set`` saw on its evaluation rows.

    ``history``: metric name -> one float per round (up to and including the round the fit
    stopped after); ``records``: the exact int64 [rounds, 4] (loss_q, n_err, n_pos, n_rows) behind
    them (logloss = loss_q / 2^30 / n_rows, error = n_err / n_rows) and ``twice_pairs`` the AUC's
    exact pair counts (auc = twice_pairs / (2 P N)), ``ap_q`` the average precision's exact integer
    sums (aucpr = ap_q / 2^30 / P, NaN without positives).  ``best_iteration`` is the first round
    with the best value of the LAST metric, ``best_score`` that value.

    With evaluation weights (``eval_sample_weight``) ``weight_q`` is the eval set's exact weight sum
    wsum_q and the records are reference_gbdt.eval_record_weighted's (loss_q, err_q, n_pos, n_rows):
    logloss = loss_q / weight_q, error = err_q / weight_q.  Without them it is None."""
    history: dict
    best_iteration: int
    best_score: float
    metrics: tuple = ("logloss",)
    records: np.ndarray | None = None
    twice_pairs: np.ndarray | None = None
    stopped: bool = False
    ap_q: np.ndarray | None = None
    weight_q: int | None = None

    @property
    def n_rounds(self) -> int:
        return int(self.records.shape[0])

    def to_dict(self) -> dict:
        return {"history": {k: [float(v) for v in vs] for k, vs in self.history.items()},
                "best_iteration": int(self.best_iteration), "best_score": float(self.best_score),
                "stopped": bool(self.stopped)}


def stop_round(keys, patience: int | None):
    """The stop rule on a sequence of exact integer keys (smaller is better): round t improves when
    its key is strictly below the best so far; the fit stops after the first round t with
    t - best >= patience.  Returns (best, stop) -- ``stop`` is None when the rule never fires."""
    best = 0
    for t in range(1, len(keys)):
        if keys[t] < keys[best]:
            best = t
        elif patience is not None and t - best >= patience:
            return best, t
    return best, None


class _Eval:
    """Evaluation state of one fit: the metrics, the exact per-round records and the stop rule.
    The CPU and the device branch of fit_binned feed it records in round order (``push``) and it
    answers whether the fit is over -- a pure function of the metric sequence."""

    def __init__(self, metrics, patience, T):
        self.metrics, self.patience, self.T = metrics, patience, T
        self.weight_q = None   # the eval set's weight sum wsum_q under evaluation weights
        self.records = np.zeros((T, 4), np.int64)
        self.twice = np.zeros(T, np.int64)
        self.apq = np.zeros(T, np.int64)
        self.done = 0          # records pushed
        self.best = 0
        self.stop_at = None    # the round the rule fired after

    @property
    def want_auc(self) -> bool:
        return "auc" in self.metrics

    @property
    def want_aucpr(self) -> bool:
        return "aucpr" in self.metrics

    def key(self, t: int) -> int:
        last = self.metrics[-1]
        if last == "aucpr":  # P is the same in every round: -ap_q orders the rounds as -AP does
            return int(-self.apq[t])
        return int(-self.twice[t]) if last == "auc" else int(self.records[t, 0 if last == "logloss" else 1])

    def push(self, rec, twice=0, ap_q=0) -> bool:
        """Record of round ``self.done``; True when the fit stops after that round."""
        t = self.done
        self.records[t] = rec
        self.twice[t] = twice
        self.apq[t] = ap_q
        self.done = t + 1
        if t == 0 or self.key(t) < self.key(self.best):
            self.best = t
        elif self.patience is not None and t - self.best >= self.patience:
            self.stop_at = t
            return True
        return False

    @property
    def n_keep(self) -> int:
        """Trees the ensemble keeps: all that were grown, or [: best + 1] under early stopping."""
        return self.best + 1 if (self.patience is not None and self.done) else self.done

    def result(self) -> EvalRecord:
        k = self.done
        rec, tw, aq = self.records[:k].copy(), self.twice[:k].copy(), self.apq[:k].copy()
        rows = np.maximum(rec[:, 3], 1).astype(np.float64)
        P = rec[:, 2].astype(np.float64)
        N = rec[:, 3].astype(np.float64) - P
        hist = {}
        for name in self.metrics:
            if name in ("logloss", "error") and self.weight_q is not None:
                v = rec[:, 0 if name == "logloss" else 1].astype(np.float64) / float(self.weight_q)
            elif name == "logloss":
                v = rec[:, 0].astype(np.float64) / R.LOSS_SCALE / rows
            elif name == "error":
                v = rec[:, 1].astype(np.float64) / rows
            elif name == "aucpr":
                with np.errstate(all="ignore"):
                    v = np.where(P > 0, aq.astype(np.float64) / R.LOSS_SCALE / P, np.nan)
            else:
                with np.errstate(all="ignore"):
                    v = np.where((P > 0) & (N > 0), tw.astype(np.float64) / (2.0 * P * N), np.nan)
            hist[name] = [float(x) for x in v]
        best_score = hist[self.metrics[-1]][self.best] if k else float("nan")
        return EvalRecord(history=hist, best_iteration=int(self.best), best_score=float(best_score),
                          metrics=tuple(self.metrics), records=rec, twice_pairs=tw if self.want_auc else None,
                          stopped=self.stop_at is not None, ap_q=aq if self.want_aucpr else None,
                          weight_q=self.weight_q)


def _eval_request(eval_set, eval_metric, early_stopping_rounds, hole_len, checkpoint, dist, T):
    """Validated (kind, Xv, yv, _Eval) of a fit's evaluation arguments, or None without eval_set."""
    if eval_set is None:
        if early_stopping_rounds is not None:
            raise ValueError("early_stopping_rounds needs an eval_set")
        return None
    if checkpoint is not None:
        raise NotImplementedError("checkpoint= cannot be combined with eval_set: a resumed fit would have to "
                                  "replay the metric history and the stop rule's state, which is not saved")
    metrics = (eval_metric,) if isinstance(eval_metric, str) else tuple(eval_metric or ("logloss",))
    bad = [m for m in metrics if m not in EVAL_METRICS]
    if bad or not metrics:
        raise ValueError(f"eval_metric must be among {EVAL_METRICS}, got {bad or metrics}")
    if "auc" in metrics and dist:
        raise NotImplementedError("eval_metric 'auc' is not supported under data-parallel training "
                                  "(pair counts do not add across ranks)")
    if "aucpr" in metrics and dist:
        raise NotImplementedError("eval_metric 'aucpr' is not supported under data-parallel training "
                                  "(the tie-group sums do not add across ranks)")
    if early_stopping_rounds is not None and int(early_stopping_rounds) < 1:
        raise ValueError("early_stopping_rounds must be >= 1")
    patience = None if early_stopping_rounds is None else int(early_stopping_rounds)
    if isinstance(eval_set, str):
        if eval_set != "hole":
            raise ValueError('eval_set is (Xv, yv) or the string "hole"')
        if not hole_len:
            raise ValueError('eval_set="hole" needs hole= (the rows left out of the fit)')
        return "hole", None, None, _Eval(metrics, patience, T)
    if isinstance(eval_set, list):
        if len(eval_set) != 1:
            raise ValueError("exactly one eval set is supported")
        eval_set = eval_set[0]
    if not (isinstance(eval_set, tuple) and len(eval_set) == 2):
        raise ValueError('eval_set is (Xv, yv) or the string "hole"')
    Xv, yv = eval_set
    if Xv.shape[0] != yv.shape[0]:
        raise ValueError("eval_set: Xv and yv disagree on the row count")
    if Xv.shape[0] > R.EVAL_MAX_ROWS:
        raise ValueError("at most 2^27 eval rows")
    return "set", Xv, yv, _Eval(metrics, patience, T)


def _resume(checkpoint, sig, T):
    """Trees of a matching checkpoint (numpy arrays) and how many rounds they cover."""
    if checkpoint is None:
        return None, 0
    got = checkpoint.latest(sig)
    if got is None:
        return None, 0
    tensors, meta = got
    t0 = min(int(meta["trees_done"]), T)
    return {k: v.numpy()[:t0] for k, v in tensors.items()}, t0


def _weights_arg(w, rows: int, dev: torch.device, name: str) -> torch.Tensor:
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or w.dim() != 1 or w.shape[0] != rows:
        raise ValueError(f"{name} must be a float32 tensor of shape [{rows}] (one weight per row)")
    if w.device != dev:
        raise ValueError(f"{name} must be on the fit's device ({dev}), got {w.device}")
    return w.contiguous()


def _weight_stats(w: torch.Tensor, y: torch.Tensor | None, ha: int, hl: int, spw: float, comm, name: str):
    """(wmax, smallest positive w_eff) of a fit's weights -- the table rows without the hole, all
    ranks -- after refusing NaN, infinite, negative and all-zero weights: one device reduction
    (gbdt.hip gbdt_weight_stats_kernel) and one host read."""
    n = int(w.shape[0])
    if not w.is_cuda:
        keep = np.r_[0:ha, ha + hl:n]
        wmax, effmin, bad = R.weight_stats(w.numpy()[keep], None if y is None else y.numpy()[keep], spw)
    else:
        out = torch.tensor([0, 0x7FF0000000000000, 0], dtype=torch.int64, device=w.device)
        native().gbdt_weight_stats(ptr(w), 0 if y is None else ptr(y), n, ha, hl, spw, ptr(out), stream_of(w))
        o = out.cpu().numpy()
        wmax = float(o[:1].astype(np.uint32).view(np.float32)[0])
        effmin, bad = float(o[1:2].view(np.float64)[0]), int(o[2])
    if comm is not None and comm.world_size > 1:  # every rank raises, or none does
        wmax = comm.all_reduce_scalar(wmax, "max")
        effmin = comm.all_reduce_scalar(effmin, "min")
        bad = int(comm.all_reduce_scalar(float(bad)))
    if bad:
        raise ValueError(f"{name} must be finite and >= 0 ({bad} entries are NaN, infinite or negative)")
    if not wmax > 0.0:
        raise ValueError(f"{name}: no row has a positive weight")
    return wmax, effmin


def fit(X: torch.Tensor, y: torch.Tensor, params: GBDTParams | None = None, comm=None,
        cuts=None, sample_weight_pos: float | None = None, return_margin: bool = False,
        checkpoint=None, checkpoint_every: int = 10, use_graph: bool | None = None,
        eval_set=None, eval_metric=("logloss",), early_stopping_rounds: int | None = None,
        row_offset: int | None = None, sample_weight: torch.Tensor | None = None,
        eval_sample_weight: torch.Tensor | None = None):
    """Boost `n_estimators` depth-D trees on standardized float32 rows X [n, d] with labels y.

    ``checkpoint``: a utils.checkpoint.CheckpointManager.  Every ``checkpoint_every`` rounds the
    trees so far are saved; a later call with the same data/config resumes after the last saved
    round.  Training margins are recomputed from the saved trees over the same bins, so a resumed
    fit is bit-identical to an uninterrupted one.

    ``eval_set`` / ``eval_metric`` / ``early_stopping_rounds`` / ``row_offset`` / ``sample_weight`` /
    ``eval_sample_weight``: see fit_binned; with an eval set the return value gains an EvalRecord as
    its last element.  The quantile cuts computed here are unweighted."""
    p = (params or GBDTParams()).validate()
    n, d = X.shape
    if d > MAX_FEAT:
        raise ValueError(f"at most {MAX_FEAT} features")
    if cuts is None:
        cuts = quantile_cuts(X, p.max_bin, p.cut_sample_rows, comm, p.learn_missing)
    bins = bin_rows(X, cuts[0], cuts[1], missing=p.learn_missing)
    return fit_binned(bins, y, cuts, p, comm=comm, sample_weight_pos=sample_weight_pos, return_margin=return_margin,
                      checkpoint=checkpoint, checkpoint_every=checkpoint_every, use_graph=use_graph,
                      eval_set=eval_set, eval_metric=eval_metric, early_stopping_rounds=early_stopping_rounds,
                      row_offset=row_offset, sample_weight=sample_weight, eval_sample_weight=eval_sample_weight)


def fit_binned(bins: torch.Tensor, y: torch.Tensor, cuts, params: GBDTParams | None = None, comm=None,
               sample_weight_pos: float | None = None, return_margin: bool = False, checkpoint=None,
               checkpoint_every: int = 10, use_graph: bool | None = None, hole: tuple | None = None,
               eval_set=None, eval_metric=("logloss",), early_stopping_rounds: int | None = None,
               row_offset: int | None = None, sample_weight: torch.Tensor | None = None,
               eval_sample_weight: torch.Tensor | None = None):
    """Boosting on already-binned rows (u8 [n, 32], bin_rows) with their cuts (cuts, nbins).

    ``hole``: (at, len) -- the fit's rows are the table without the block [at, at + len) (a
    cross-validation fold on the fold-sorted table: no per-fold copy).  The returned margin (with
    ``return_margin``) covers EVERY table row, so the block's margins are the fold's validation
    scores under the fitted ensemble.

    ``eval_set``: ``(Xv, yv)`` -- standardized float32 rows (binned here with the fit's cuts) or
    already-binned u8 [m, 32] rows, with uint8 labels -- or the string ``"hole"``: the hole's rows,
    whose margins every round's walk keeps current anyway.  Exactly one eval set.  After every round
    the metrics of ``eval_metric`` ("logloss", "error", "auc", "aucpr") are taken on it as exact
    integers (gbdt.hip gbdt_eval_kernel; EvalRecord).  "aucpr" is sklearn's average precision over
    the tie groups of the margins (auc.hip, ops/metrics.average_precision_device); xgboost's
    ``aucpr`` interpolates the curve slightly differently, so its values differ a little.  Without
    ``early_stopping_rounds`` this changes nothing about the trees.
    With it, the LAST metric drives the stop rule (as in xgboost): a round improves
    when its integer sum is strictly better than the best so far, and the fit stops after the first
    round t with t - best >= early_stopping_rounds.  The host waits for round t - patience's record
    before it enqueues round t, so at most ``early_stopping_rounds`` rounds are in flight and the
    decision does not depend on timing.  The ensemble then keeps trees [: best_iteration + 1] --
    xgboost keeps the later trees in the booster and merely never predicts with them -- and the
    returned margin is rebuilt from the kept trees by the round's own margin kernel, so it equals
    their walk bit for bit.  With an eval set the return value gains an EvalRecord as its last
    element.  Under data-parallel training every rank passes its shard of the eval rows and the
    integer records are all-reduced, so all ranks stop at the same round.

    Stochastic boosting (``subsample``, ``colsample_bytree`` / ``_bylevel`` / ``_bynode``, ``seed`` of
    GBDTParams): round t's trees see the gradients of the sampled rows only -- an out-of-sample row's
    quantised (g, h) is 0, so it adds nothing to any histogram -- and a node's split scan may pick
    only the node's sampled features.  Every table row still takes every tree's margin update, and
    evaluation, early stopping and the returned margins are those of the full rows, as in xgboost.
    The draws are stateless Philox functions of (seed, round, global row id | feature)
    (reference_gbdt.row_sample_mask / feature_masks), so repeated fits and resumed fits are bitwise
    equal and a fold keeps its draws around a ``hole`` (a row keeps its TABLE index).  ``row_offset``:
    the global id of table row 0; None is 0, or under ``comm`` the sum of the lower ranks' table
    rows, so contiguous shards in rank order grow the single-process trees.  The feature masks of
    all rounds are drawn on the host and uploaded once; no round waits for the host.  With any
    sampling on, the opt-in hipGraph path (FDX_GBDT_GRAPH=1 / use_graph) and FDX_GBDT_FUSE_MARGIN=1
    fall back to the eager, unfused round: the round number t, which selects the row sample and the
    row of the mask table, is a launch argument that changes every round: a captured graph would
    replay the value of the round it was recorded in, and the fused level-0 pass (gbdt_hist_l0_fused)
    computes the gradients itself and has no sampled variant.

    Per-row weights (``sample_weight``): a float32 [n] tensor on the bins' device, one weight per
    TABLE row, finite and >= 0 with at least one positive among the fit's rows (entries inside a
    ``hole`` are ignored for training).  A row's effective weight is w_eff = w * (y ? scale_pos_weight
    : 1), and its gradient pair g = (p - y) w_eff, h = max(p (1 - p), 1e-16) w_eff is formed in fp64
    before the quantisation; histograms, split scan, partition and leaves work on the integers as
    before, bitwise deterministic.  The fixed-point scale is gscale = 2^floor(log2(2^14 / W)), W =
    max(scale_pos_weight, 1) * wmax with wmax the largest weight over the fit's rows (all ranks; one
    device reduction and one host read per fit, no round waits for the host), hscale = 4 gscale: an
    all-ones fit is the unweighted fit bit for bit.  Resolution: the packed (g, h) word has 14 bits,
    so a row with w_eff * gscale < 16 has fewer than 16 quanta of gradient even at |p - y| = 1 and
    its contribution is coarsely rounded; the fit issues one UserWarning naming the ratio when the
    smallest positive w_eff is that far (more than 2^10) below the largest.  A row of weight 0 stays
    in the table, takes every margin update and every partition and adds nothing to any histogram;
    with ``subsample`` an out-of-sample row's word is 0 whatever its weight.  The quantile cuts stay
    unweighted (xgboost's sketch is Hessian-weighted).  With weights, as under sampling, the
    hipGraph path and FDX_GBDT_FUSE_MARGIN=1 fall back to the eager, unfused round
    (gbdt_hist_l0_fused has no weighted variant).  ``checkpoint=`` with ``sample_weight`` raises
    NotImplementedError: the signature would have to cover the weights.

    Missing values (``missing_policy="learn"`` of GBDTParams): byte 255 of a binned row is the missing
    slot (bin_rows(..., missing=True); the cuts hold at most 255 real bins), the split scan learns for
    every split which side the slot's rows take, and the ensemble carries the choice in
    ``default_left`` (reference_gbdt's module docstring has the rules; the device matches it
    bitwise).  Histograms, leaves, gradients, sampling, weights and evaluation are what they were.
    On the device the direction travels inside the round's ``bin`` words (encode_bin_words), so
    partition, margin and eval walks need no further argument; the host decodes them when it copies
    the trees back and encodes them again on a checkpoint resume.  Float eval rows are binned with
    the same rule.  Under "learn" FDX_GBDT_FUSE_MARGIN=1 falls back to the eager, unfused round, as
    under sampling and weights: the fused level-0 pass (gbdt_hist_l0_fused) has its own walk, which
    knows no directions.  The hipGraph path replays the same kernels and needs nothing.

    Evaluation weights (``eval_sample_weight``, xgboost's sample_weight_eval_set): float32 [m] for an
    ``(Xv, yv)`` set, [hole_len] for ``eval_set="hole"``, finite and >= 0 with a positive entry.
    "logloss" and "error" become weighted means and stay exact integers
    (reference_gbdt.eval_record_weighted; EvalRecord.weight_q is the denominator); the stop rule
    compares the integer numerators, the denominator being constant.  "auc" and "aucpr" with
    evaluation weights raise NotImplementedError (their kernels count pairs and tie groups).

    Monotone constraints (``monotone_constraints`` of GBDTParams, xgboost's TreeEvaluator in fp64;
    reference_gbdt's module docstring has the rules): every heap node carries weight bounds, a side's
    weight is clamped into them, a candidate on a constrained feature must order its children's
    weights, and the children of such a split meet at the mean of their weights.  Only the split scan
    and the leaf weights change, both fp64 functions of the integer histogram sums, so trees stay
    bitwise deterministic and equal to the oracle's, and a constrained tree is an ordinary tree for
    every walk, explainer and model file.  Every tree -- and so the fp32 margin, fp32 addition being
    monotone in each argument -- is monotone in every constrained feature over its non-NaN values.
    The bounds live in two static workspace arrays (the hipGraph path replays them); sampling,
    weights, learned missing directions, evaluation, the row hole, data parallelism (the histograms
    are all-reduced before the scan) and checkpoints compose unchanged.  The length is checked
    against the feature count here; all zero is the unconstrained fit, launch for launch.

    Interaction constraints (``interaction_constraints`` of GBDTParams, xgboost's
    FeatureInteractionConstraintHost; reference_gbdt's module docstring has the rules): a list of
    groups of feature indices, which may overlap.  Every heap node carries ``path``, the set of
    features its ancestors split on; with an empty path every feature is eligible, otherwise the
    path's own features and every group that contains the whole path -- a feature in no group is only
    followed by itself.  The split features are chosen on the device, so the split kernel carries the
    path words down the heap itself (one static uint32 workspace array; the group masks travel in the
    kernel arguments, so the hipGraph path replays them) and ANDs the allowed set into the word that
    column sampling already gates candidates with: the sample is drawn first, then filtered, and a
    node left with nothing does not split.  Only eligibility changes -- gain arithmetic, tie order and
    acceptance are untouched, trees stay bitwise equal to the oracle's, and a constrained tree is an
    ordinary tree for every walk, explainer and model file.  Indices are checked against the feature
    count here; at most 32 groups; None, [] or only empty groups is the unconstrained fit, launch for
    launch.

    L1 regularisation and the weight cap (``reg_alpha`` and ``max_delta_step`` of GBDTParams, xgboost's
    names; reference_gbdt's module docstring has the rules): with a = reg_alpha a side's weight is
    -T(G) / (H + lambda), T the soft threshold of G at a, capped to +-max_delta_step where that is
    positive and only then clamped into the monotone bounds; a side's gain term is twice the
    reduction of the regularised objective G w + (H + lambda) w^2 / 2 + a |w| at that weight, whatever
    clamped it.  Only the split scan and the leaf weights change, both fp64 functions of the integer
    histogram sums: the two values travel by value in the arguments of gbdt_split and gbdt_leaf (the
    hipGraph path replays them), trees stay bitwise equal to the oracle's, every leaf satisfies
    |leaf| <= float32(learning_rate * max_delta_step), and a = 2 n max(scale_pos_weight, 1) or more
    leaves every tree empty.  The fused level-0 pass runs no scan and is unaffected; sampling, weights,
    learned missing directions, monotone and interaction constraints, evaluation, the row hole, data
    parallelism (the scan sees all-reduced histograms) and checkpoints compose unchanged.  Both 0 is
    the fit without them, launch for launch; model files and checkpoint signatures name the two only
    off their defaults."""
    p = (params or GBDTParams()).validate()
    cuts_np, nbins = cuts
    d = int(len(nbins))
    n = int(bins.shape[0])  # table rows (the margin walk covers all of them)
    if d > MAX_FEAT:
        raise ValueError(f"at most {MAX_FEAT} features")
    if y.dtype != torch.uint8 or y.shape[0] != n:
        raise ValueError("y must be uint8 [n] (one label per table row)")
    ha, hl = (int(hole[0]), int(hole[1])) if hole else (0, 0)
    if ha < 0 or hl < 0 or ha + hl > n:
        raise ValueError(f"hole {hole} outside the {n} table rows")
    n_fit = n - hl
    spw = float(p.scale_pos_weight if sample_weight_pos is None else sample_weight_pos)
    wt, wmax = None, 1.0
    if sample_weight is not None:
        if checkpoint is not None:
            raise NotImplementedError("checkpoint= cannot be combined with sample_weight: the checkpoint's "
                                      "signature does not cover the weights")
        wt = _weights_arg(sample_weight, n, bins.device, "sample_weight")
        wmax, eff_min = _weight_stats(wt, y, ha, hl, spw, comm, "sample_weight")
    gscale, hscale = R.grad_scales(spw, wmax)
    if wt is not None and eff_min * gscale < R.WEIGHT_MIN_QUANTA:
        warnings.warn(f"sample_weight: the smallest positive effective weight {eff_min:.3g} times the gradient "
                      f"scale {gscale:g} is {eff_min * gscale:.3g} < {R.WEIGHT_MIN_QUANTA:g}: such rows have fewer "
                      f"than {R.WEIGHT_MIN_QUANTA:g} quanta of gradient (14-bit fixed point, largest effective "
                      f"weight {max(spw, 1.0) * wmax:.3g})", UserWarning, stacklevel=2)
    D = p.max_depth
    ni, nl = (1 << D) - 1, 1 << D
    T = p.n_estimators
    base_margin = float(np.log(p.base_score / (1.0 - p.base_score)))
    dist = comm is not None and comm.world_size > 1
    sub_on, seed = p.subsample != 1.0, int(p.seed)
    learn = p.learn_missing
    mono = p.monotone_signs(d)  # [d] signs or None
    mono_inc = 0 if mono is None else int(sum(1 << f for f in range(d) if mono[f] > 0))
    mono_dec = 0 if mono is None else int(sum(1 << f for f in range(d) if mono[f] < 0))
    inter = p.interaction_masks(d)  # group masks or None
    inter_named = None if inter is None else [list(g) for g in p.interaction_constraints]
    reg = p.reg  # (reg_alpha, max_delta_step) or None
    if learn and int(np.max(nbins, initial=0)) > MAX_BIN - 1:
        raise ValueError('missing_policy="learn": byte 255 is the missing slot, the cuts may hold at most 255 '
                         "real bins per feature (quantile_cuts(..., missing=True))")
    thresh = R.sample_threshold(p.subsample) if sub_on else 0
    if row_offset is None:
        row_offset = 0
        if sub_on and dist:
            row_offset = int(sum(r[0] for r in comm.all_gather_ints([n])[:comm.rank]))
    row_offset = int(row_offset)
    if row_offset < 0 or row_offset + n >= 1 << 62:
        raise ValueError("row_offset must be >= 0 (and the global row ids below 2^62)")
    # allowed-feature bits of every (round, heap node), drawn on the host once per fit
    fmasks = R.feature_mask_table(seed, T, d, D, p.colsample_bytree, p.colsample_bylevel,
                                  p.colsample_bynode) if p.colsampled else None
    # the policy is named only where it is not the default: a "last_bin" model serialises as before
    ens_kw = dict(depth=D, cuts=cuts_np, nbins=nbins, base_score=p.base_score,
                  params={**{k: v for k, v in p.__dict__.items()
                             if k not in ("missing_policy", "monotone_constraints", "interaction_constraints",
                                          "reg_alpha", "max_delta_step")
                             or (k == "missing_policy" and learn)},
                          **({} if not float(p.reg_alpha) else {"reg_alpha": float(p.reg_alpha)}),
                          **({} if not float(p.max_delta_step) else {"max_delta_step": float(p.max_delta_step)}),
                          "seed": seed, **({} if mono is None else {"monotone_constraints": [int(c) for c in mono]}),
                          **({} if inter is None else {"interaction_constraints": inter_named})})
    req = _eval_request(eval_set, eval_metric, early_stopping_rounds, hl, checkpoint,
                        comm is not None and comm.world_size > 1, T)
    ev = None
    if req is not None:
        ev_kind, Xv, yv, ev = req
        if ev_kind == "set":
            if yv.dtype != torch.uint8 or yv.device != bins.device or Xv.device != bins.device:
                raise ValueError("eval_set: yv must be uint8, and Xv, yv on the fit's device")
            if Xv.dtype == torch.uint8:
                if Xv.dim() != 2 or Xv.shape[1] != R.ROW_BYTES:
                    raise ValueError("eval_set: binned rows must be u8 [m, 32]")
                bins_v = Xv.contiguous()
            else:
                if Xv.dim() != 2 or Xv.shape[1] != d:
                    raise ValueError(f"eval_set: the fit has {d} features, Xv has {tuple(Xv.shape)}")
                bins_v = bin_rows(Xv if Xv.is_cuda else Xv.float(), cuts_np, nbins, missing=learn)
            yv = yv.contiguous()
    w_ev = None
    if eval_sample_weight is not None:
        if ev is None:
            raise ValueError("eval_sample_weight needs an eval_set")
        if ev.want_auc or ev.want_aucpr:
            raise NotImplementedError("eval_metric 'auc' / 'aucpr' do not take evaluation weights "
                                      "(their kernels count pairs and tie groups); use 'logloss' or 'error'")
        w_ev = _weights_arg(eval_sample_weight, hl if ev_kind == "hole" else int(yv.shape[0]), bins.device,
                            "eval_sample_weight")
        ev_wscale = R.eval_weight_scale(_weight_stats(w_ev, None, 0, 0, 1.0, comm, "eval_sample_weight")[0])
        # wsum_q, a constant of the eval set: an exact int64 sum, once per fit
        wq = torch.round(w_ev.double() * (ev_wscale * R.EVAL_WEIGHT_SCALE)).to(torch.int64).sum().reshape(1)
        ev.weight_q = int((comm.all_reduce(wq) if dist else wq).item())
    sig = None
    if checkpoint is not None:
        from ..utils.checkpoint import config_signature

        n_all = int(comm.all_reduce_scalar(float(n_fit))) if (comm is not None and comm.world_size > 1) else n_fit
        # the sampling fields only where they differ from their defaults: checkpoints written before
        # they existed still resume
        dflt = p.SAMPLING_DEFAULTS
        sig_params = {k: v for k, v in p.__dict__.items()
                      if k not in ("n_estimators", "monotone_constraints", "interaction_constraints")
                      and not (k in dflt and v == dflt[k])}
        if mono is not None:  # the resolved signs, whatever form they were given in
            sig_params["monotone_constraints"] = [int(c) for c in mono]
        if inter is not None:  # the resolved groups
            sig_params["interaction_constraints"] = inter_named
        # Which global rows the fit draws for is part of a sampled fit's configuration.  Every rank
        # must compute the SAME signature (rank 0 writes the checkpoint, all ranks load it), so
        # under data parallelism it names every rank's offset, not this rank's.
        offs = {}
        if sub_on and dist:
            offs = {"row_offsets": [int(r[0]) for r in comm.all_gather_ints([row_offset])]}
        elif sub_on and row_offset:
            offs = {"row_offset": row_offset}
        sig = config_signature(params=sig_params, spw=spw,
                               cuts=cuts_np, nbins=nbins, n=n_all, d=d, **({"hole": [ha, hl]} if hl else {}), **offs)
    prev, t0 = _resume(checkpoint, sig, T)

    def _save(t_done, feat, binv, thr, gain, leaf, dleft=None):
        if checkpoint is not None and t_done > 0:
            extra = {} if dleft is None else {"default_left": dleft[:t_done]}
            checkpoint.save(t_done, {"feat": feat[:t_done], "bin": binv[:t_done], "thr": thr[:t_done],
                                     "gain": gain[:t_done], "leaf": leaf[:t_done], **extra},
                            {"signature": sig, "trees_done": t_done, "kind": "gbdt"})
            fault = os.environ.get("FDX_FAULT", "")
            if fault.startswith("gbdt_crash_after_trees=") and t_done >= int(fault.split("=", 1)[1]):
                os._exit(17)  # simulated lost rank right after a checkpoint (resume tests)

    if not bins.is_cuda:
        feat = np.zeros((T, ni), np.int32); binv = np.zeros((T, ni), np.int32)
        thr = np.zeros((T, ni), np.float32); gain = np.zeros((T, ni)); leaf = np.zeros((T, nl), np.float32)
        dleft = np.zeros((T, ni), np.uint8) if learn else None
        b_all = bins.numpy()
        y_all = y.numpy()
        keep = np.r_[0:ha, ha + hl:n]
        b, yy = b_all[keep], y_all[keep]
        ww = None if wt is None else wt.numpy()[keep]
        margin = np.full(n_fit, np.float32(base_margin), np.float32)
        if t0:
            feat[:t0], binv[:t0], thr[:t0], gain[:t0], leaf[:t0] = (prev[k] for k in ("feat", "bin", "thr", "gain", "leaf"))
            if learn:
                dleft[:t0] = prev["default_left"]
            margin = R.predict_margin_bins(b, feat[:t0], binv[:t0], leaf[:t0], D, base_margin,
                                           None if dleft is None else dleft[:t0])
        if ev is not None:  # the eval rows' bins, labels and running margin (the device's eval walk)
            b_ev, y_ev = (b_all[ha:ha + hl], y_all[ha:ha + hl]) if ev_kind == "hole" else (bins_v.numpy(), yv.numpy())
            m_ev = np.full(b_ev.shape[0], np.float32(base_margin), np.float32)
        for t in range(t0, T):
            q = R.gradients(margin, yy, spw, gscale, hscale, ww)
            if sub_on:  # global ids of the fit's rows: a row keeps its table index around the hole
                q[~R.row_sample_mask(seed, t, keep + row_offset, p.subsample)] = 0
            tr, node = R.build_tree(b, q, cuts_np, nbins, D, p.reg_lambda, p.min_child_weight, p.gamma,
                                    p.learning_rate, gscale, hscale, comm, None if fmasks is None else fmasks[t],
                                    learn, mono, inter, reg)
            feat[t], binv[t], thr[t], gain[t], leaf[t] = tr.feat, tr.bin, tr.thr, tr.gain, tr.leaf
            if learn:
                dleft[t] = tr.default_left
            margin = (margin + tr.leaf[node]).astype(np.float32)
            if (t + 1) % max(1, checkpoint_every) == 0 or t + 1 == T:
                _save(t + 1, feat, binv, thr, gain, leaf, dleft)
            if ev is not None:
                m_ev = (m_ev + R.predict_margin_bins(b_ev, feat[t:t + 1], binv[t:t + 1], leaf[t:t + 1], D, 0.0,
                                                     None if dleft is None else dleft[t:t + 1])
                        ).astype(np.float32)
                rec = R.eval_record(m_ev, y_ev) if w_ev is None else \
                    R.eval_record_weighted(m_ev, y_ev, w_ev.numpy(), ev_wscale)
                if comm is not None and comm.world_size > 1:
                    rec = comm.all_reduce(torch.from_numpy(rec)).numpy()
                if ev.push(rec, R.twice_pairs(m_ev, y_ev) if ev.want_auc else 0,
                           R.ap_q(m_ev, y_ev) if ev.want_aucpr else 0):
                    break
        if ev is not None and ev.n_keep < T:  # early stop: keep [: best + 1], margins of the kept trees
            k = ev.n_keep
            feat, binv, thr, gain, leaf = feat[:k], binv[:k], thr[:k], gain[:k], leaf[:k]
            dleft = None if dleft is None else dleft[:k]
            margin = R.predict_margin_bins(b, feat, binv, leaf, D, base_margin, dleft)
        ens = TreeEnsemble(feat=feat, bin=binv, thr=thr, gain=gain, leaf=leaf, default_left=dleft, **ens_kw)
        tail = () if ev is None else (ev.result(),)
        if not return_margin:
            return (ens, *tail) if tail else ens
        full = np.empty(n, np.float32)
        full[keep] = margin
        if hl:
            full[ha:ha + hl] = R.predict_margin_bins(b_all[ha:ha + hl], feat, binv, leaf, D, base_margin, dleft)
        return (ens, torch.from_numpy(full), *tail)

    m = native()
    dev = bins.device
    st0 = stream_of(bins)
    ws = _Workspace(n, D, dev)
    # feature-major copy of the bins for the partition's one-byte-per-row reads (gbdt.hip)
    ldt = max(4, (n + 255) // 256 * 256)
    binsT = torch.empty(d * ldt, dtype=torch.uint8, device=dev)
    if n:
        m.gbdt_transpose(ptr(bins), n, d, ptr(binsT), ldt, st0)
    n_global = int(comm.all_reduce_scalar(float(n_fit))) if dist else n_fit
    ct = torch.from_numpy(np.ascontiguousarray(cuts_np[:d])).to(dev)
    nt = torch.from_numpy(np.ascontiguousarray(nbins[:d])).to(dev)
    feat = torch.empty((T, ni), dtype=torch.int32, device=dev)
    binv = torch.empty((T, ni), dtype=torch.int32, device=dev)
    thr = torch.empty((T, ni), dtype=torch.float32, device=dev)
    gain = torch.empty((T, ni), dtype=torch.float64, device=dev)
    leaf = torch.empty((T, nl), dtype=torch.float32, device=dev)
    margin = torch.full((n,), base_margin, dtype=torch.float32, device=dev)
    if t0:
        if learn:  # the device's bin words carry the direction
            prev = {**prev, "bin": encode_bin_words(prev["bin"], prev["default_left"])}
        for name, dst in (("feat", feat), ("bin", binv), ("thr", thr), ("gain", gain), ("leaf", leaf)):
            dst[:t0].copy_(torch.from_numpy(np.ascontiguousarray(prev[name])))
        for t in range(t0):  # the margins of the saved trees, by the round's own margin kernel
            m.gbdt_margin(ptr(binsT), ldt, n, ptr(feat[t]), ptr(binv[t]), ptr(leaf[t]), D, ptr(margin), ptr(y), spw,
                          gscale, hscale, 0, st0)
    lam, mcw, gam = float(p.reg_lambda), float(p.min_child_weight), float(p.gamma)
    ginv, hinv = 1.0 / gscale, 1.0 / hscale
    # [T, ni] uint32 bits, rows contiguous: a split launch gets the address of its round's row
    fm_dev = torch.from_numpy(np.ascontiguousarray(fmasks).view(np.int32)).to(dev) if fmasks is not None else None

    def round_body(o_feat, o_bin, o_thr, o_gain, o_leaf, grad_first=False, grad_next=True, prev=None,
                   defer_margin=False, t=0):
        """One boosting round: a fixed launch sequence with static pointers (graph-capturable).
        The gradients of a round come from the previous round's margin update (gbdt_margin with
        gh), so only the first round of a fit launches gbdt_grad.  ``prev`` (feat, bin, leaf of the
        previous tree, its margin walk deferred): level 0 runs that walk fused in front of its
        histogram (gbdt_hist_l0_fused).  ``defer_margin``: leave this tree's walk to the next round.
        ``t``: the round, read only under sampling (round t's row sample goes into the gradients
        that round t - 1's margin walk writes; round t's feature masks into its split scans)."""
        st = stream_of(bins)  # the capture stream while a hipGraph is being recorded
        if grad_first and wt is not None and sub_on:
            m.gbdt_grad_sampled_weighted(ptr(margin), ptr(y), ptr(wt), n, spw, gscale, hscale, ptr(ws.gh), seed, t,
                                         row_offset, thresh, st)
        elif grad_first and wt is not None:
            m.gbdt_grad_weighted(ptr(margin), ptr(y), ptr(wt), n, spw, gscale, hscale, ptr(ws.gh), st)
        elif grad_first and sub_on:
            m.gbdt_grad_sampled(ptr(margin), ptr(y), n, spw, gscale, hscale, ptr(ws.gh), seed, t, row_offset, thresh, st)
        elif grad_first:
            m.gbdt_grad(ptr(margin), ptr(y), n, spw, gscale, hscale, ptr(ws.gh), st)
        # zero histograms and per-node counts, root segment + global count: one launch (level 0
        # reads rows in order, so ridx / nid need no iota / root fill)
        m.gbdt_round_init(ptr(ws.hist), ws.hist.numel(), ptr(ws.seg), ptr(ws.gcnt), n_fit, n_global, st,
                          ptr(ws.node_r), ws.node_r.numel())
        cur = 0
        fmask_arg = () if fm_dev is None else (ptr(fm_dev[t]),)  # the round's [ni] mask row; none: every feature
        miss_arg = {"missing": True} if learn else {}  # the scan learns the missing slot's side; o_bin gets words
        # monotone fit: the sign masks and the heap's weight bounds (static pointers)
        mono_arg = {} if mono is None else {"mono_inc": mono_inc, "mono_dec": mono_dec, "mono_lo": ptr(ws.blo),
                                            "mono_hi": ptr(ws.bhi)}
        # interaction constraints: the group masks (constants) and the heap's path words (static pointer)
        inter_arg = {} if inter is None else {"inter_groups": inter, "inter_path": ptr(ws.path)}
        # reg_alpha / max_delta_step: two constants of the split scan and the leaf weights
        reg_arg = {} if reg is None else {"reg_alpha": reg[0], "max_delta_step": reg[1]}
        for level in range(D):
            h0, nn = (1 << level) - 1, 1 << level
            if level == 0 and prev is not None:
                m.gbdt_hist_l0_fused(ptr(bins), ptr(ws.gh), ptr(ws.seg), ptr(ws.gcnt), d, ptr(ws.hist), ptr(ws.slots),
                                     st, HIST_FLUSH_ROWS, ha, hl, ptr(prev[0]), ptr(prev[1]), ptr(prev[2]), D,
                                     ptr(margin), ptr(y), spw, gscale, hscale)
            else:
                m.gbdt_hist(ptr(bins), ptr(ws.gh), ptr(ws.ridx[cur]), ptr(ws.seg), ptr(ws.gcnt), level, d,
                            ptr(ws.hist), ptr(ws.slots), st, HIST_FLUSH_ROWS, ha, hl)
            if dist:
                comm.all_reduce_(ws.hist[h0 * HIST_ENTRIES:(h0 + nn) * HIST_ENTRIES])
            m.gbdt_split(ptr(ws.hist), ptr(ws.gcnt), level, d, ptr(nt), ptr(ct), ginv, hinv, lam, mcw, gam,
                         ptr(o_feat), ptr(o_bin), ptr(o_thr), ptr(o_gain), ptr(ws.ng), ptr(ws.nh), st, *fmask_arg,
                         **miss_arg, **mono_arg, **inter_arg, **reg_arg)
            if level == D - 1:
                break  # leaves: the margin walk and gbdt_leaf (split-kernel child sums) need no partition
            if n_fit:
                # count + scatter; the scatter also writes the children's segments and counts (gcnt)
                m.gbdt_partition(ptr(binsT), ldt, ptr(ws.ridx[cur]), ptr(ws.nid[cur]), n_fit, ptr(o_feat), ptr(o_bin),
                                 level, ptr(ws.flag), ptr(ws.counts), PART_BLOCKS, ptr(ws.seg), ptr(ws.node_r),
                                 ptr(ws.ridx[cur ^ 1]), ptr(ws.nid[cur ^ 1]), st, ptr(ws.gcnt), ha, hl)
            cur ^= 1
            c0 = 2 * h0 + 1
            if not n_fit:
                ws.seg[2 * h0 + 1:2 * (h0 + nn) + 1].zero_()
                ws.gcnt[c0:c0 + 2 * nn].zero_()
            if dist:
                comm.all_reduce_(ws.gcnt[c0:c0 + 2 * nn])
        m.gbdt_leaf(ptr(ws.ng), ptr(ws.nh), D, ginv, hinv, lam, mcw, float(p.learning_rate), ptr(o_leaf), st,
                    *((ptr(ws.blo), ptr(ws.bhi)) if mono is not None else ()), **reg_arg)
        if n and not defer_margin and grad_next and wt is not None and sub_on:
            m.gbdt_margin_sampled_weighted(ptr(binsT), ldt, n, ptr(o_feat), ptr(o_bin), ptr(o_leaf), D, ptr(margin),
                                           ptr(y), ptr(wt), spw, gscale, hscale, ptr(ws.gh), seed, t + 1, row_offset,
                                           thresh, st)
        elif n and not defer_margin and grad_next and wt is not None:
            m.gbdt_margin_weighted(ptr(binsT), ldt, n, ptr(o_feat), ptr(o_bin), ptr(o_leaf), D, ptr(margin), ptr(y),
                                   ptr(wt), spw, gscale, hscale, ptr(ws.gh), st)
        elif n and not defer_margin and grad_next and sub_on:
            m.gbdt_margin_sampled(ptr(binsT), ldt, n, ptr(o_feat), ptr(o_bin), ptr(o_leaf), D, ptr(margin), ptr(y), spw,
                                  gscale, hscale, ptr(ws.gh), seed, t + 1, row_offset, thresh, st)
        elif n and not defer_margin:
            m.gbdt_margin(ptr(binsT), ldt, n, ptr(o_feat), ptr(o_bin), ptr(o_leaf), D, ptr(margin), ptr(y), spw,
                          gscale, hscale, ptr(ws.gh) if grad_next else 0, st)

    def after_round(t):
        if checkpoint is not None and ((t + 1) % max(1, checkpoint_every) == 0 or t + 1 == T):
            if learn:  # checkpoints hold bin / default_left, not the device's words
                dl = (binv[:t + 1] >> 9) == 1
                _save(t + 1, feat, torch.where(dl, (binv[:t + 1] & 0x1FF) - 1, binv[:t + 1]), thr, gain, leaf,
                      dl.to(torch.uint8))
                return
            _save(t + 1, feat, binv, thr, gain, leaf)  # device -> host copy: syncs every k rounds only

    # hipGraph: a round is ~5 + 6*D launches with static shapes, so after one eager round it is
    # recorded once and replayed (one graph launch per round instead of ~45 Python->HIP launches;
    # the per-round tree lands in a fixed record and is copied into its slot).  Not under DP,
    # where the round contains host-side collectives.  Opt-in (FDX_GBDT_GRAPH=1): eager launches
    # already run ahead of the GPU, and replay + record copies measured 0.61 vs 0.50 ms/tree at
    # 0.96M rows and 1.62 vs 1.54 at 6.4M (profiles/r1_s22).
    if use_graph is None:  # opt-in: measured slower than eager launches (profiles/r1_s22)
        use_graph = os.environ.get("FDX_GBDT_GRAPH", "0") == "1"
    # Evaluation keeps the eager launches: a round is followed by the eval kernel, a record copy and
    # an event, and the stop rule may end the fit between two rounds.  The deferred margin walk is
    # off too (the hole's margins must be current when the round's record is taken).
    # Sampling keeps them too, unfused: a recorded round and the fused level-0 pass bake the round's
    # constants in, and the round number (row sample, mask row) is one of them.
    # Per-row weights keep them as well: the fused level-0 pass has no weighted variant.
    # missing_policy="learn" drops the fused pass only (its walk knows no directions).
    graphable = use_graph and not dist and n > 0 and T - t0 >= 3 and ev is None and not p.sampled and wt is None
    fuse_margin = (os.environ.get("FDX_GBDT_FUSE_MARGIN", "0") == "1" and not graphable and ev is None
                   and not p.sampled and wt is None and not learn)
    graph = None
    if ev is not None:
        from . import metrics as metric_ops

        # device history, zeroed once (the kernel adds into a round's row); pinned host mirror the
        # round's record is copied into on the fit's stream, with one event per round
        ev_hist = torch.zeros((T, 4), dtype=torch.int64, device=dev)
        ev_host = torch.empty((T, 4), dtype=torch.int64).pin_memory()
        ev_done = [None] * T
        if ev_kind == "set":
            nv = int(bins_v.shape[0])
            ldt_v = max(4, (nv + 255) // 256 * 256)
            binsT_v = torch.empty(d * ldt_v, dtype=torch.uint8, device=dev)
            if nv:
                m.gbdt_transpose(ptr(bins_v), nv, d, ptr(binsT_v), ldt_v, st0)
            m_ev, y_ev = torch.full((nv,), base_margin, dtype=torch.float32, device=dev), yv
        else:
            m_ev, y_ev = margin[ha:ha + hl], y[ha:ha + hl]  # views: the training walk keeps them current
        if ev.want_auc:
            ev_tw = torch.zeros(T, dtype=torch.int64, device=dev)
            tw_host = torch.zeros(T, dtype=torch.int64).pin_memory()
            ev_pos = int(y_ev.sum(dtype=torch.int64).item())  # the positive count, read once
        if ev.want_aucpr:
            ev_ap = torch.zeros(T, dtype=torch.int64, device=dev)
            ap_host = torch.zeros(T, dtype=torch.int64).pin_memory()
            ap_ws = metric_ops.pr_workspace(int(m_ev.shape[0]), dev)  # the sort's scratch, once per fit

        def eval_round(t):
            st = stream_of(bins)
            if ev_kind == "set" and w_ev is not None:
                m.gbdt_eval_walk_weighted(ptr(binsT_v), ldt_v, nv, ptr(feat[t]), ptr(binv[t]), ptr(leaf[t]), D,
                                          ptr(m_ev), ptr(y_ev), ptr(w_ev), ev_wscale, ptr(ev_hist[t]), st)
            elif ev_kind == "set":
                m.gbdt_eval_walk(ptr(binsT_v), ldt_v, nv, ptr(feat[t]), ptr(binv[t]), ptr(leaf[t]), D, ptr(m_ev),
                                 ptr(y_ev), ptr(ev_hist[t]), st)
            elif w_ev is not None:
                # the kernel indexes the weights by TABLE row like margin and label: hole row r reads
                # w_ev[r - ha], so the pointer is moved back by ha entries (never read below the hole)
                m.gbdt_eval_weighted(ptr(margin), ptr(y), ptr(w_ev) - 4 * ha, ev_wscale, ha, ha + hl, ptr(ev_hist[t]), st)
            else:
                m.gbdt_eval(ptr(margin), ptr(y), ha, ha + hl, ptr(ev_hist[t]), st)
            if dist:
                comm.all_reduce_(ev_hist[t])
            ev_host[t].copy_(ev_hist[t], non_blocking=True)
            if ev.want_auc:
                _, twice = metric_ops.auc_known_positives(m_ev, y_ev, ev_pos)
                ev_tw[t].copy_(twice)
                tw_host[t:t + 1].copy_(ev_tw[t:t + 1], non_blocking=True)
            if ev.want_aucpr:
                _, ap_res = metric_ops.average_precision_device(m_ev, y_ev, ws=ap_ws)
                ev_ap[t].copy_(ap_res[0])
                ap_host[t:t + 1].copy_(ev_ap[t:t + 1], non_blocking=True)
            ev_done[t] = torch.cuda.Event()
            ev_done[t].record()

        def eval_take(s):
            """Wait for round s's record and apply the stop rule to it."""
            ev_done[s].synchronize()
            return ev.push(ev_host[s].numpy(), int(tw_host[s]) if ev.want_auc else 0,
                           int(ap_host[s]) if ev.want_aucpr else 0)

    rounds_run = t0
    for t in range(t0, T):
        if ev is not None and ev.patience is not None and t - ev.patience >= 0 and eval_take(t - ev.patience):
            break
        rounds_run = t + 1
        if graphable and t == t0 + 1:  # round t0 ran eagerly: its kernels had to execute
            from ..runtime.graphs import capture

            rec = [torch.empty(ni, dtype=torch.int32, device=dev), torch.empty(ni, dtype=torch.int32, device=dev),
                   torch.empty(ni, dtype=torch.float32, device=dev), torch.empty(ni, dtype=torch.float64, device=dev),
                   torch.empty(nl, dtype=torch.float32, device=dev)]
            graph = capture(lambda: round_body(*rec))
        if graph is not None:
            graph.replay()
            for dst, src in zip((feat[t], binv[t], thr[t], gain[t], leaf[t]), rec):
                dst.copy_(src)
        else:
            # FDX_GBDT_FUSE_MARGIN=1: a round's margin walk runs fused into the next round's level-0
            # histogram pass (one pass over the table fewer) -- measured slower: 410 us for the fused
            # pass against 151 + 140 us (its per-row fp64 phase and the LANE phase alternate behind
            # block barriers, 64-VGPR budget, profiles/r6_gbdt), so opt-in
            fuse = fuse_margin and n_fit > 0
            round_body(feat[t], binv[t], thr[t], gain[t], leaf[t], grad_first=(t == t0), grad_next=(t + 1 < T),
                       prev=(feat[t - 1], binv[t - 1], leaf[t - 1]) if (fuse and t > t0) else None,
                       defer_margin=fuse and t + 1 < T, t=t)
        after_round(t)
        if ev is not None:
            eval_round(t)
    def host_bins(words):  # (bin, default_left) of the device's split words
        return decode_bin_words(words.cpu().numpy()) if learn else (words.cpu().numpy(), None)

    if ev is None:
        bin_np, dl_np = host_bins(binv)
        ens = TreeEnsemble(feat=feat.cpu().numpy(), bin=bin_np, thr=thr.cpu().numpy(),
                           gain=gain.cpu().numpy(), leaf=leaf.cpu().numpy(), default_left=dl_np, **ens_kw)
        return (ens, margin) if return_margin else ens
    # the records still in flight, in round order (the rule may fire on one of them: the rounds
    # enqueued past it are dropped, exactly as if the host had seen the record in time)
    while ev.stop_at is None and ev.done < rounds_run:
        eval_take(ev.done)
    k = ev.n_keep
    if return_margin and k < rounds_run and n:
        # margins of the kept trees, by the round's own margin kernel (as the checkpoint resume)
        margin.fill_(base_margin)
        for t in range(k):
            m.gbdt_margin(ptr(binsT), ldt, n, ptr(feat[t]), ptr(binv[t]), ptr(leaf[t]), D, ptr(margin), ptr(y), spw,
                          gscale, hscale, 0, st0)
    bin_np, dl_np = host_bins(binv[:k])
    ens = TreeEnsemble(feat=feat[:k].cpu().numpy(), bin=bin_np, thr=thr[:k].cpu().numpy(),
                       gain=gain[:k].cpu().numpy(), leaf=leaf[:k].cpu().numpy(), default_left=dl_np, **ens_kw)
    return (ens, margin, ev.result()) if return_margin else (ens, ev.result())


# ---- inference -------------------------------------------------------------------------------
class DeviceEnsemble:
    """Tree arrays resident on a device for repeated inference."""

    def __init__(self, ens: TreeEnsemble, device: torch.device):
        self.ens = ens
        self.device = device
        self.feat = torch.from_numpy(np.ascontiguousarray(ens.feat)).to(device)
        self.thr = torch.from_numpy(np.ascontiguousarray(ens.thr)).to(device)
        self.leaf = torch.from_numpy(np.ascontiguousarray(ens.leaf)).to(device)
        # None: no node sends a NaN left (gbdt_predict's null pointer, the walk it always did)
        self.dleft = torch.from_numpy(np.ascontiguousarray(ens.default_left, np.uint8)).to(device) \
            if ens.has_default_left else None


def predict_margin(X: torch.Tensor, ens: TreeEnsemble, dens: DeviceEnsemble | None = None,
                   n_trees: int | None = None) -> torch.Tensor:
    """float32 margins of standardized rows X [n, d] (d <= 30, any row stride).  ``n_trees``: use
    only the first n_trees trees (the ensemble after that many boosting rounds)."""
    n, d = X.shape
    if d != ens.n_features:
        raise ValueError(f"model has {ens.n_features} features, X has {d}")
    k = ens.n_trees if n_trees is None else int(n_trees)
    if not 0 <= k <= ens.n_trees:
        raise ValueError(f"n_trees must be in [0, {ens.n_trees}]")
    if not X.is_cuda:
        return torch.from_numpy(R.predict_margin(X.numpy(), ens.feat[:k], ens.thr[:k], ens.leaf[:k], ens.depth,
                                                 ens.base_margin,
                                                 ens.default_left[:k] if ens.has_default_left else None))
    if X.dtype != torch.float32 or X.stride(1) != 1:
        raise ValueError("X must be float32 with unit column stride")
    dens = dens if dens is not None and dens.device == X.device else DeviceEnsemble(ens, X.device)
    out = torch.empty(n, dtype=torch.float32, device=X.device)
    if n:
        native().gbdt_predict(ptr(X), n, X.stride(0), d, ptr(dens.feat), ptr(dens.thr), ptr(dens.leaf), k,
                              ens.depth, ens.base_margin, ptr(out), stream_of(X),
                              *((ptr(dens.dleft),) if getattr(dens, "dleft", None) is not None else ()))
    return out


def predict_proba(X: torch.Tensor, ens: TreeEnsemble, dens: DeviceEnsemble | None = None,
                  n_trees: int | None = None) -> torch.Tensor:
    return torch.sigmoid(predict_margin(X, ens, dens, n_trees))


# ---- node covers -----------------------------------------------------------------------------
def tree_cover_chunk(depth: int) -> int:
    """Trees whose nodes and int64 leaf sums one tree_cover launch keeps in LDS (the launcher's
    chunk): (32768 - 1024) // ((2 (2^D - 1) + 2^D) 4 + 2^D 8)."""
    return int(native().tree_cover_chunk_trees(int(depth)))


def node_cover(X: torch.Tensor, ens: TreeEnsemble, kind: str = "hessian",
               dens: DeviceEnsemble | None = None) -> torch.Tensor:
    """int64 [T, 2^(D+1)] node covers of ``ens`` over the standardized rows X [n, d] (fp32, d <= 30,
    any row stride), by 1-based heap node; reference_gbdt.node_cover has the definitions.  Device
    rows run csrc/kernels/treecover.hip, CPU rows the numpy oracle.  ``TreeEnsemble.with_cover``
    stores the result in a model.  The sums are integers, so per-rank tables of a data-parallel
    run would simply add; that all-reduce is not wired up."""
    if kind not in R.COVER_KINDS:
        raise ValueError(f"cover kind must be one of {R.COVER_KINDS}, not {kind!r}")
    n, d = X.shape
    if d != ens.n_features:
        raise ValueError(f"model has {ens.n_features} features, X has {d}")
    if int(ens.feat.max(initial=-1)) >= d or int(ens.feat.min(initial=0)) < -1:
        raise ValueError("the ensemble's split features do not fit the rows' width")
    dl = ens.default_left if ens.has_default_left else None
    if not X.is_cuda:
        return torch.from_numpy(R.node_cover(X.numpy(), ens.feat, ens.thr, ens.leaf, ens.depth, ens.base_margin, dl,
                                             kind))
    if X.dtype != torch.float32 or X.stride(1) != 1:
        raise ValueError("X must be float32 with unit column stride")
    if not 1 <= ens.depth <= 8:
        raise ValueError("node_cover supports depth 1..8")
    dens = dens if dens is not None and dens.device == X.device else DeviceEnsemble(ens, X.device)
    out = torch.empty((ens.n_trees, 2 << ens.depth), dtype=torch.int64, device=X.device)
    need_ws = kind == "hessian" and ens.n_trees > tree_cover_chunk(ens.depth) and n > 0
    ws = torch.empty(n, dtype=torch.float32, device=X.device) if need_ws else None
    native().tree_cover(ptr(X) if n else 0, n, X.stride(0) if n else d, d, ptr(dens.feat), ptr(dens.thr),
                        ptr(dens.leaf), ptr(dens.dleft) if getattr(dens, "dleft", None) is not None else 0,
                        ens.n_trees, ens.depth, float(ens.base_margin), 1 if kind == "hessian" else 0,
                        ptr(ws) if ws is not None else 0, ptr(out), stream_of(X))
    return out
