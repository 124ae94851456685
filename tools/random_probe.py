"""GPU box: the symmetric random baseline (gsparse.random) as the device form against
the host form it replaces (the reference's NumPy lines, GSPARSE_RANDOM=host).

On R-MAT-SCALE, with edge_index on the host and on the device: the wall time of
precompute_random_scores, of one random_sparsify (r = 0.5, arrays uploaded) and of a
5-rate RandomBaseline.sweep (handle built outside the clock), each as a warm-up and then
the median of REPS runs, torch synchronised inside the clock; that both forms give the
same arrays; and the per-kernel times of gs_undirected_ids (keys, sort, scan, scatter)
and of the gather, from the context profiler in a run of their own.

usage: random_probe.py [SCALE] [REPS] [OUT.json]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "gnn-sparsification-research_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gsparse  # noqa: E402
from gsparse import graphs  # noqa: E402
from gsparse import random as R  # noqa: E402

scale = int(sys.argv[1]) if len(sys.argv) > 1 else 18
reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else None
RATES = [0.9, 0.7, 0.5, 0.3, 0.1]

ei = graphs.rmat(scale, 8, seed=0)
n = 1 << scale
E = int(ei.shape[1])
out = {"workload": f"RMAT-{scale} symmetric random baseline", "nodes": n, "E": E, "reps": reps,
       "rates": RATES, "cases": []}


def median_s(fn):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    print(f"# median of {reps}: {statistics.median(ts):.6f} s", file=sys.stderr, flush=True)
    return statistics.median(ts), res


def form(name):
    os.environ["GSPARSE_RANDOM"] = name


for where in ("host", "device"):
    t = torch.from_numpy(ei)
    data = gsparse.Data(edge_index=t.cuda() if where == "device" else t, num_nodes=n)
    dev = "cuda:0" if where == "device" else "cpu"
    case = {"edge_index": where, "output": dev}
    res = {}
    for f in ("host", "device"):
        form(f)
        case[f"precompute_{f}_s"], (us, inv) = median_s(lambda: R.precompute_random_scores(data, 42))
        assert R.last_selection["path"] == f
        case[f"sparsify_{f}_s"], sd = median_s(lambda: R.random_sparsify(data, us, inv, 0.5, dev))
        assert R.last_selection["path"] == f
        rb = gsparse.RandomBaseline(data, seed=42)
        case[f"sweep_{f}_s"], sw = median_s(lambda: rb.sweep(RATES, dev))
        assert rb.last_selection["path"] == f
        res[f] = (us, inv, sd.edge_index.cpu().numpy(), [s.edge_index.cpu().numpy() for s in sw])
    h, d = res["host"], res["device"]
    case["n_undirected"] = int(len(h[0]))
    case["equal"] = bool(np.array_equal(h[0].view(np.uint64), d[0].view(np.uint64))
                         and np.array_equal(h[1], d[1]) and np.array_equal(h[2], d[2])
                         and all(np.array_equal(a, b) for a, b in zip(h[3], d[3])))
    for k in ("precompute", "sparsify", "sweep"):
        case[f"{k}_host_over_device"] = case[f"{k}_host_s"] / case[f"{k}_device_s"]
    out["cases"].append(case)
    print(json.dumps(case), flush=True)

# kernel times in a run of their own: the profiler's events bracket every launch
form("device")
t = torch.from_numpy(ei).cuda()
data = gsparse.Data(edge_index=t, num_nodes=n)
eng = R._engine(data, None)
inv_d = torch.empty(E, dtype=torch.int64, device="cuda")
eng.undirected_ids(t[0], t[1], n, out=inv_d)
rb = gsparse.RandomBaseline(data, seed=42)
eng.ctx.profile(True)
eng.ctx.profile_reset()
for _ in range(reps):
    eng.undirected_ids(t[0], t[1], n, out=inv_d)
    rb.mask(0.5)
prof = eng.ctx.profile_read()
eng.ctx.profile(False)
out["kernels"] = {k: {"ms": v["ms"] / max(1, v["launches"]), "bytes": v["bytes"] / max(1, v["launches"]),
                      "GBps": (v["bytes"] / 1e9) / (v["ms"] / 1e3) if v["ms"] > 0 else None}
                  for k, v in prof.items()}
print(json.dumps(out["kernels"]), flush=True)

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
