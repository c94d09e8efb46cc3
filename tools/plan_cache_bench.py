#!/usr/bin/env python3
"""What a plan file saves: for the stand-ins at full size, the time of create (Tuning::None and
Tuning::Aggressive), of save and of load (the file in the page cache), and the file size -- all on the
same box, in the same run.  Writes profiles/plan_cache.json.

    python tools/plan_cache_bench.py [--scale 1.0] [--out profiles/plan_cache.json] [name:dtype ...]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT = ["Flan_1565:f64", "Queen_4147:f32", "ldoor:f64", "pwtk:f64", "powerlaw:f64"]
NO_CALIBRATE = 32


def timed(f):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", default=DEFAULT)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_cache.json"))
    args = ap.parse_args()
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import synth
    torch.cuda.init()
    torch.cuda.set_device(0)
    rows = []
    with tempfile.TemporaryDirectory() as d:
        for case in args.cases:
            name, dt = case.split(":")
            dtype = np.float64 if dt == "f64" else np.float32
            n, rp, ci, va = synth.generate(name, args.scale)[:4]
            va = va.astype(dtype)
            row = {"matrix": name, "dtype": dt, "scale": args.scale, "n": int(n), "nnz": int(rp[-1])}
            for label, flags in (("none", NO_CALIBRATE), ("aggressive", 0)):
                A, t_create = timed(lambda: cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=flags)))
                path = os.path.join(d, f"{name}.{dt}.{label}.plan")
                _, t_save = timed(lambda: A.save(path))
                B, t_load = timed(lambda: cfs.SymMatrix.load(path))  # (just written: in the page cache)
                B.close()
                B, t_load2 = timed(lambda: cfs.SymMatrix.load(path))
                row[label] = {"create_s": t_create, "save_s": t_save, "load_s": min(t_load, t_load2),
                              "file_bytes": os.path.getsize(path), "device_bytes": A.stats()["device_bytes"],
                              "same_digest": A.digest() == B.digest()}
                A.close(), B.close()
                os.remove(path)
            print(json.dumps(row), flush=True)
            rows.append(row)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/plan_cache_bench.py", "cases": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
