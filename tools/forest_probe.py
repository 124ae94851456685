"""GPU box: what the maximum spanning forest (gs_spanning_forest) costs, on one graph with
device Jaccard scores, edge list and scores resident on the device.

Each as a warm-up and then the median of REPS (>= 10) runs, torch synchronised inside the
clock: the forest alone (expand = 0), the expanded forest (expand = 1, with
gs_undirected_ids), gs_components and gs_topk_mask (r = 0.5) on the same graph, and
SciPy's minimum_spanning_tree on the host (its own run count: it takes seconds).  Then, in
runs of their own, the context profiler's split into the ranking (keys, sort, gather of
the ends) and the rounds, and the rounds' list lengths from GSPARSE_FOREST_DEBUG, against
the edge list's size.

usage: forest_probe.py GRAPH [REPS] [OUT.json] [SCIPY_RUNS]
GRAPH: roman (the full Roman-like graph), rmatK (R-MAT scale K)"""
import json
import os
import re
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "gnn-sparsification-research_amd"))
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402
from scipy.sparse.csgraph import minimum_spanning_tree  # noqa: E402

from gsparse import graphs  # noqa: E402
from gsparse._lib import Context  # noqa: E402
from gsparse.engine import Engine  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "roman"
reps = max(10, int(sys.argv[2])) if len(sys.argv) > 2 else 10
out_path = sys.argv[3] if len(sys.argv) > 3 else None
scipy_runs = int(sys.argv[4]) if len(sys.argv) > 4 else 1

if name == "roman":
    ei, n = graphs.roman_like(), 22662
else:
    scale = int(name[4:])
    ei, n = graphs.rmat(scale, 8, seed=0), 1 << scale
ei = np.ascontiguousarray(ei, dtype=np.int64)
E = int(ei.shape[1])

ctx = Context(0)
ctx.set_graph_edge_index(n, ei[0], ei[1])
eng = Engine(ctx)
assert eng.nnz == E, "one score per column is needed"
t = torch.from_numpy(ei).cuda()
s = torch.empty(E, dtype=torch.float64, device="cuda")
eng.jaccard(out=s)
mask = torch.empty(E, dtype=torch.uint8, device="cuda")
out = {"graph": name, "nodes": n, "E": E, "reps": reps, "edge_list_bytes": 16 * E, "score_bytes": 8 * E}


def median_s(fn, runs=reps, warm=True):
    if warm:
        fn()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), res


out["forest_s"], out["forest_min_s"], (_, lab, info) = median_s(
    lambda: eng.spanning_forest(s, t[0], t[1], n, False, False, out=mask))
forest_bytes = mask.cpu().numpy().tobytes()
out["expanded_s"], out["expanded_min_s"], (_, _, info_x) = median_s(
    lambda: eng.spanning_forest(s, t[0], t[1], n, False, True, out=mask))
out.update(n_forest=info["n_forest"], rounds=info["rounds"], n_guaranteed=info_x["n_marked"])
out["components_s"], out["components_min_s"], (_, ncomp, _) = median_s(eng.components)
out["components"] = ncomp
assert info["n_forest"] == n - ncomp
out["topk_s"], out["topk_min_s"], _ = median_s(lambda: eng.topk_mask(s, E, E // 2, False, out=mask))
out["forest_over_components"] = out["forest_s"] / out["components_s"]
out["forest_over_topk"] = out["forest_s"] / out["topk_s"]
print(json.dumps(out), flush=True)

# the profiler's split, in runs of its own
ctx.profile(True)
ctx.profile_reset()
for _ in range(reps):
    eng.spanning_forest(s, t[0], t[1], n, False, True, out=mask)
prof = ctx.profile_read()
ctx.profile(False)
out["phases"] = {k: {"ms_per_call": v["ms"] / reps, "launches_per_call": v["launches"] / reps,
                     "bytes_per_call": v["bytes"] / reps,
                     "GBps": (v["bytes"] / 1e9) / (v["ms"] / 1e3) if v["ms"] > 0 else None}
                 for k, v in prof.items() if k.startswith(("forest_", "undirected_"))}
print(json.dumps(out["phases"]), flush=True)

# the rounds' list lengths: the library's own trace, read back from its stderr
os.environ["GSPARSE_FOREST_DEBUG"] = "1"
sys.stderr.flush()
with tempfile.TemporaryFile() as tmp:
    keep = os.dup(2)
    os.dup2(tmp.fileno(), 2)
    try:
        eng.spanning_forest(s, t[0], t[1], n, False, False, out=mask)
    finally:
        os.dup2(keep, 2)
        os.close(keep)
    tmp.seek(0)
    trace = tmp.read().decode()
del os.environ["GSPARSE_FOREST_DEBUG"]
assert mask.cpu().numpy().tobytes() == forest_bytes, "two runs differ"


def round_bytes(rnd, listed, crossing):
    """The list (the first round's is implicit), its ends and their labels, the survivors
    written; per node its label, pick, hook and jump."""
    return (16 if rnd == 0 else 20) * listed + 4 * crossing + 40 * n


out["round_trace"] = [
    {"round": int(m[1]), "list": int(m[2]), "crossing": int(m[3]), "hooked": int(m[4]), "jump_passes": int(m[5]),
     "bytes": round_bytes(int(m[1]), int(m[2]), int(m[3])),
     "bytes_over_edge_list": round_bytes(int(m[1]), int(m[2]), int(m[3])) / (16 * E)}
    for m in re.finditer(r"round=(\d+) list=(\d+) crossing=(\d+) hooked=(\d+) jump_passes=(\d+)", trace)]
print(json.dumps(out["round_trace"]), flush=True)

# SciPy on the host: the undirected graph with the scores as weights (distinct pairs only)
if scipy_runs > 0:
    sh = s.cpu().numpy()
    lo, hi = np.minimum(ei[0], ei[1]), np.maximum(ei[0], ei[1])
    nl = lo != hi
    a = sp.coo_matrix((-(sh[nl] + 1.0), (lo[nl], hi[nl])), shape=(n, n)).tocsr()
    a.data[:] = np.minimum(a.data, -1.0)  # duplicates were summed: any negative weight will do for the time
    out["scipy_mst_s"], _, tree = median_s(lambda: minimum_spanning_tree(a), runs=scipy_runs, warm=False)
    out["scipy_tree_edges"] = int(tree.nnz)
    out["scipy_over_forest"] = out["scipy_mst_s"] / out["forest_s"]
    print(json.dumps({k: out[k] for k in ("scipy_mst_s", "scipy_tree_edges", "scipy_over_forest")}), flush=True)

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
