#!/usr/bin/env python3
"""k-NN (SMOTE self-search, k=5) at the bench shapes: engines x candidate slices.

    python tools/knn_lab.py [--reps 20] [--engines fp32,bf16x3r,bf16x3t,bf16x3f] [--json out.json]

Shapes: DP1 (the 10M-row bench's 13.6k minority rows against themselves) and the DP=8 global-scope
rank (its 13.6k minority rows against all 8 ranks' 108.8k).  For every nsplit the event-timed
median of the whole knn_topk call (prep + search + merge) and whether the lists equal the
auto-split lists exactly.  For bf16x3f nsplit is the waves of a workgroup (clamped to the launcher's
limit) and --caps sweeps its LDS list cap per query.  (r4: a pilot search seeding every slice's threshold was measured here
too, 1-3% slower at every split count -- profiles/r4_g/knn_lab.json -- and removed.)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--splits", default="1,2,4,8,16,32")
    ap.add_argument("--engines", default="fp32")
    ap.add_argument("--caps", default="", help="bf16x3f: list caps to time at the auto wave count, e.g. 16,32,64,128")
    ap.add_argument("--alternate", default=None, metavar="ENG[:NSPLIT],...",
                    help="also time these engines one call each in turn, --reps rounds (medians per engine)")
    a = ap.parse_args()
    from fraud_detection_amd.data.synthetic import separable
    from fraud_detection_amd.ops import knn as K
    from fraud_detection_amd.ops.native import native

    dev = torch.device("cuda", 0)
    m1, world = 13600, 8
    X, y = separable(2 * m1 * world + 4096, fraud_rate=0.5, seed=5, device=dev)
    xm = X[y == 1][: m1 * world]
    xm = (xm - X.mean(0)) / X.std(0)
    C = torch.zeros((xm.shape[0], 32), device=dev)
    C[:, :30] = xm
    C[:, 30] = 1.0
    shapes = {"dp1_self": (C[:m1].contiguous(), C[:m1].contiguous(), 0),
              "dp8_global_rank3": (C[3 * m1: 4 * m1].contiguous(), C, 3 * m1)}
    out = {"reps": a.reps, "flush": os.environ.get("FDX_KNN_FLUSH", "4"), "shapes": {}}

    def timed(fn):
        for _ in range(3):
            fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.reps + 1)]
        ev[0].record()
        for i in range(a.reps):
            fn()
            ev[i + 1].record()
        torch.cuda.synchronize()
        return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(a.reps)]))

    splitter = {"fp32": "knn_splits", "bf16x3r": "knn3r_splits", "bf16x3t": "knn3t_splits", "bf16x3f": "knn3f_waves"}
    for name, (Q, Cc, off) in shapes.items():
        mq, mc = Q.shape[0], Cc.shape[0]
        ref = K.knn_topk(Q, Cc, 5, off, engine="fp32")
        for eng in a.engines.split(","):
            auto = getattr(native(), splitter[eng])((mq + 31) // 32 * 32, (mc + 31) // 32 * 32)
            rec = {"engine": eng, "mq": mq, "mc": mc, "auto_nsplit": int(auto), "cases": []}
            splits = {int(v) for v in a.splits.split(",")} | {int(auto)}
            if eng == "bf16x3f":
                splits = {min(v, int(native().KNN3F_MAX_WAVES)) for v in splits}
            for ns in sorted(splits):
                f = lambda: K.knn_topk(Q, Cc, 5, off, engine=eng, nsplit=ns)  # noqa: E731
                got = f()
                ms = timed(f)
                if eng != "fp32":
                    dg = {}
                    K.knn_topk(Q, Cc, 5, off, engine=eng, nsplit=ns, _diag=dg)
                    dg.pop("counts", None)
                    dg.pop("scanned", None)
                    print(json.dumps({name: {"engine": eng, "nsplit": ns, "lists": dg}}), flush=True)
                case = {"engine": eng, "nsplit": ns, "ms": round(ms, 4),
                        "lists_match_frac": float((got == ref).all(1).float().mean().item()),
                        "tflops_equiv": round(2.0 * mq * mc * 32 / (ms * 1e-3) / 1e12, 1),
                        "lists_equal": bool((got == ref).all().item())}
                rec["cases"].append(case)
                print(json.dumps({name: case}), flush=True)
            if eng == "bf16x3f":
                for cap in (int(v) for v in a.caps.split(",") if v):
                    f = lambda: K.knn_topk(Q, Cc, 5, off, engine=eng, nsplit=int(auto), list_cap=cap)  # noqa: E731
                    got = f()
                    dg = {}
                    K.knn_topk(Q, Cc, 5, off, engine=eng, nsplit=int(auto), list_cap=cap, _diag=dg)
                    case = {"engine": eng, "nsplit": int(auto), "list_cap": cap, "ms": round(timed(f), 4),
                            "exact_scans": dg["exact_scans"], "lists_equal": bool((got == ref).all().item())}
                    rec.setdefault("caps", []).append(case)
                    print(json.dumps({name: case}), flush=True)
            best = min(rec["cases"], key=lambda c: c["ms"])
            base = [c for c in rec["cases"] if c["nsplit"] == auto][0]
            rec["best"], rec["auto"] = best, base
            out["shapes"][f"{name}:{eng}"] = rec
    if a.alternate:
        # one call of each engine per round, so drift of the card's clocks hits all of them alike
        spec = [(e.split(":")[0], int(e.split(":")[1]) if ":" in e else None) for e in a.alternate.split(",")]
        for name, (Q, Cc, off) in shapes.items():
            fns = [(lambda e=e, ns=ns: K.knn_topk(Q, Cc, 5, off, engine=e, nsplit=ns)) for e, ns in spec]
            for f in fns:
                for _ in range(3):
                    f()
            ms = [[] for _ in spec]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.reps * len(spec) + 1)]
            ev[0].record()  # queued back to back (no host sync in between), as ``timed`` does
            for r in range(a.reps):
                for i, f in enumerate(fns):
                    f()
                    ev[r * len(spec) + i + 1].record()
            torch.cuda.synchronize()
            for r in range(a.reps):
                for i in range(len(spec)):
                    ms[i].append(ev[r * len(spec) + i].elapsed_time(ev[r * len(spec) + i + 1]))
            rec = {f"{e}:{ns if ns else 'auto'}": {"median_ms": round(float(np.median(v)), 4),
                                                   "min_ms": round(float(np.min(v)), 4)}
                   for (e, ns), v in zip(spec, ms)}
            out["shapes"][f"{name}:alternate"] = rec
            print(json.dumps({name: {"alternate": rec}}), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
