"""GPU box: what the Simmelian backbone (gs_simmelian) costs against the support pass it
starts from (gs_common_neighbors), on one graph resident on the device, in both modes,
and where the time goes.

After one warm-up of each, REPS (>= 5) rounds in which gs_common_neighbors, the
non-parametric score (max_rank 0) and the overlap at max_rank RANK are timed one after the
other, so that the forms alternate; the host clock around a call that ends in a stream
synchronise; the medians with the minima and maxima are reported, the ratio of each median
to the support pass's, the pairs per class, and -- from one more profiled call per mode --
the library's own per-stage times (gs_profile: the support pass, the segment ranks, the
tables and every class kernel).  Two calls of a mode must give the same bytes.

usage: simmelian_probe.py GRAPH [REPS] [OUT.json] [RANK=5]
GRAPH: roman (the full Roman-like graph), citation (the full citation-like graph),
       rmatK (R-MAT scale K)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "gnn-sparsification-research_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gsparse import graphs  # noqa: E402
from gsparse._lib import Context  # noqa: E402
from gsparse.engine import Engine  # noqa: E402


def graph(name):
    if name == "roman":
        return graphs.roman_like(), 22662
    if name == "citation":
        return graphs.citation_like(), 169343
    scale = int(name[4:])
    return graphs.rmat(scale, 8, seed=0), 1 << scale


name = sys.argv[1] if len(sys.argv) > 1 else "roman"
reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else None
rank = int(sys.argv[4]) if len(sys.argv) > 4 else 5

ei, n = graph(name)
ei = np.ascontiguousarray(ei, dtype=np.int64)
ctx = Context(0)
ctx.set_graph_edge_index(n, ei[0], ei[1])
eng = Engine(ctx)
nnz = eng.nnz
out = {"graph": name, "nodes": n, "entries": nnz, "reps": reps, "rank": rank}
buf = torch.empty(nnz, dtype=torch.float64, device="cuda")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


modes = {"score": 0, "overlap": rank}
eng.common_neighbors(out=buf)  # warm-up: the Jaccard plan, the code objects
for label, k0 in modes.items():
    info = eng.simmelian(k0, out=buf)[1]
    first = buf.cpu().numpy()
    assert eng.simmelian(k0, out=buf)[1] == info and buf.cpu().numpy().tobytes() == first.tobytes(), label
    out[f"info_{label}"] = info
    out[f"nonzero_entries_{label}"] = int(np.count_nonzero(first))
ts = {"support": [], **{label: [] for label in modes}}
for _ in range(reps):
    ts["support"].append(timed(lambda: eng.common_neighbors(out=buf))[0])
    for label, k0 in modes.items():
        ts[label].append(timed(lambda: eng.simmelian(k0, out=buf))[0])
sup = statistics.median(ts["support"])
for label, v in ts.items():
    out[f"{label}_s"], out[f"{label}_min_s"], out[f"{label}_max_s"] = statistics.median(v), min(v), max(v)
    out[f"{label}_over_support"] = statistics.median(v) / sup
ctx.profile(True)
for label, k0 in modes.items():
    ctx.profile_reset()
    eng.simmelian(k0, out=buf)
    ctx.synchronize()
    out[f"stages_ms_{label}"] = {k: round(v["ms"], 4) for k, v in ctx.profile_read().items()}
ctx.profile(False)
print(json.dumps(out))
if out_path:
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
