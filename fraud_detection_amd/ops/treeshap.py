"""K7b interventional TreeSHAP device wrapper (csrc/kernels/treeshap.hip): exact SHAP values of a
tree ensemble's margin (log-odds) against a background set, one workgroup per explanation; and the
wrappers of the two background-free kernels on the model's node covers, path-dependent TreeSHAP
(csrc/kernels/treeshap_path.hip) and its SHAP interaction values (csrc/kernels/treeshap_interact.hip)."""
from __future__ import annotations

import math

import numpy as np
import torch

from .kernelshap import _check_x, _outputs
from .native import native, ptr, stream_of


def _device_design(expl, dev, kind):
    """The explainer's arrays on the device, cached on it per (kind, device): kind "background" adds the
    background rows' direction bits, kind "path" the child fractions and the default directions."""
    key = (kind, str(dev))
    if expl._dev_cache is not None and expl._dev_cache[0] == key:
        return expl._dev_cache[1]
    from .scaler import stats_from_numpy

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)

    ens = expl.ens
    t = {"feat": up(ens.feat, np.int32), "thr": up(ens.thr, np.float32), "leaf": up(ens.leaf, np.float32),
         "stats": stats_from_numpy(expl.mean, expl.scale, device=dev)}
    if kind == "path":
        t["frac"] = up(expl.frac, np.float32)  # fp64 rounded once
        t["dleft"] = up(ens.default_left, np.uint8) if getattr(ens, "has_default_left", False) else None
    else:
        t["bw"] = torch.from_numpy(np.ascontiguousarray(expl.bw).view(np.int32)).to(dev)
    expl._dev_cache = (key, t)
    return t


def _explain(X, expl, kind, outs, launch, sync):
    """What the three wrappers share after their checks: standardize X on the device, call
    ``launch(design, Xs [E, 32], E)`` unless E = 0, and return ``outs`` (device tensors, f0 last)
    as they are or, if ``sync``, as float64 numpy arrays with the explainer's f0."""
    E = X.shape[0]
    if E:
        from .scaler import scale_cast

        t = _device_design(expl, X.device, kind)
        launch(t, scale_cast(X, t["stats"], out_dtype="f32"), E)
    if not sync:
        return outs
    return (*(o.cpu().numpy().astype(np.float64, copy=False) for o in outs[:-1]), float(expl.f0))


def treeshap_path_lds_resident(d: int, n_trees: int, depth: int) -> bool:
    """Whether launch_treeshap_path keeps leaves, split features and fractions in LDS."""
    return bool(native().treeshap_path_trees_in_lds(int(d), int(n_trees), int(depth)))


def treeshap_path(X: torch.Tensor, expl, sync: bool = True, out=None):
    """Path-dependent TreeSHAP (csrc/kernels/treeshap_path.hip).  X [E, d] RAW fp32 on device
    (standardized on device with the model's scaler; a NaN stays NaN and follows default_left)
    -> (phi [E, d], margin(x) [E], f0): phi sums to margin(x) - f0, f0 = the explainer's expected
    value.  Numpy if ``sync`` else device tensors (``out``: preallocated (phi, fx, f0) device
    tensors).  E = 0 launches nothing and returns empty results of these shapes."""
    _check_x(X, expl.d)
    ens = expl.ens
    phi, fx, f0 = outs = _outputs(X.shape[0], expl.d, X.device, out)

    def launch(t, Xs, E):
        native().treeshap_path(ptr(Xs), Xs.stride(0), E, expl.d, ptr(t["feat"]), ptr(t["thr"]), ptr(t["leaf"]),
                               ptr(t["frac"]), ptr(t["dleft"]), ens.n_trees, ens.depth, float(ens.base_margin),
                               float(expl.f0), ptr(phi), ptr(fx), ptr(f0), stream_of(X))

    return _explain(X, expl, "path", outs, launch, sync)


def treeshap_interactions_lds_resident(d: int, n_trees: int, depth: int) -> bool:
    """Whether launch_treeshap_interactions keeps leaves, split features and fractions in LDS."""
    return bool(native().treeshap_interactions_trees_in_lds(int(d), int(n_trees), int(depth)))


def leaf_exponent(leaf) -> int:
    """The smallest integer e with max |leaf| <= 2^e (0 for an all-zero model): the fixed-point
    sums of treeshap_interact.hip are in units of 2^(e - 46).  ValueError on a non-finite leaf."""
    v = np.abs(np.asarray(leaf, np.float64))
    if not np.all(np.isfinite(v)):
        raise ValueError("SHAP interaction values need finite leaf values")
    vmax = float(v.max()) if v.size else 0.0
    if vmax == 0.0:
        return 0
    mant, ex = math.frexp(vmax)          # vmax = mant * 2^ex, 0.5 <= mant < 1
    return ex - 1 if mant == 0.5 else ex


def treeshap_interactions(X: torch.Tensor, expl, sync: bool = True, out=None, *, stream_trees: bool = False):
    """SHAP interaction values of the path-dependent game (csrc/kernels/treeshap_interact.hip).
    X [E, d] RAW fp32 on device (standardized on device with the model's scaler; a NaN stays NaN
    and follows default_left) -> (inter [E, d, d], phi [E, d], margin(x) [E], f0): inter[e] is
    symmetric bit for bit, its row i sums to phi[e, i] and the whole matrix to margin(x) - f0.
    Float64 numpy if ``sync`` else device tensors (inter float64, the rest float32; ``out``:
    preallocated (inter, phi, fx, f0) device tensors).  E = 0 launches nothing and returns empty
    results of these shapes.  ``stream_trees`` reads the per-tree constants from L2 even where they
    fit in LDS: the same result bit for bit (the sums are integers), there for tests and timing."""
    _check_x(X, expl.d)
    E, d = X.shape[0], expl.d
    ens = expl.ens
    e2 = leaf_exponent(ens.leaf)
    if out is not None:
        inter, phi, fx, f0 = out
        if (inter.shape != (E, d, d) or inter.dtype != torch.float64 or not inter.is_contiguous()
                or phi.shape != (E, d) or not phi.is_contiguous() or fx.shape[0] != E or f0.shape[0] < E):
            raise ValueError("out = (inter [E, d, d] float64 contiguous, phi [E, d] contiguous, fx [E], f0 [E]) "
                             "device tensors")
    else:
        inter = torch.empty((E, d, d), device=X.device, dtype=torch.float64)
        phi, fx, f0 = _outputs(E, d, X.device, None)

    def launch(t, Xs, E):
        native().treeshap_interactions(ptr(Xs), Xs.stride(0), E, d, ptr(t["feat"]), ptr(t["thr"]), ptr(t["leaf"]),
                                       ptr(t["frac"]), ptr(t["dleft"]), ens.n_trees, ens.depth,
                                       float(ens.base_margin), float(expl.f0), e2, bool(stream_trees), ptr(inter),
                                       ptr(phi), ptr(fx), ptr(f0), stream_of(X))

    return _explain(X, expl, "path", (inter, phi, fx, f0), launch, sync)


def treeshap(X: torch.Tensor, expl, sync: bool = True, out=None):
    """X [E, d] RAW fp32 on device (standardized on device with the model's scaler) -> (phi [E, d],
    margin(x) [E], f0): phi sums to margin(x) - f0, f0 = mean background margin.  Numpy if
    ``sync`` else device tensors (``out``: preallocated (phi, fx, f0) device tensors)."""
    _check_x(X, expl.d)
    ens = expl.ens
    phi, fx, f0 = outs = _outputs(X.shape[0], expl.d, X.device, out)

    def launch(t, Xs, E):
        native().treeshap(ptr(Xs), Xs.stride(0), E, expl.d, ptr(t["feat"]), ptr(t["thr"]), ptr(t["leaf"]),
                          ens.n_trees, ens.depth, float(ens.base_margin), ptr(t["bw"]), expl.bw.shape[1],
                          expl.B.shape[0], float(expl.f0), ptr(phi), ptr(fx), ptr(f0), stream_of(X))

    return _explain(X, expl, "background", outs, launch, sync)
