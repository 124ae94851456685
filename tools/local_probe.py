"""GPU box: what the segment ranks (gs_segment_rank) and the local-filter scores
(gs_local_scores) cost on one graph, ids and scores resident on the device, by the
library's own profiling hooks (device events around each unit's launches).

Per run one Engine.local_scores call with the profiler on; after WARM warm-up runs the
default path and GSPARSE_SEGR_MODE=sort alternate for REPS runs each.  Per profile entry:
the median, the minimum and the maximum of the per-run times, the unit's algorithmic bytes
and their rate at the median against the measured HBM copy rate (6.29 TB/s).  "rank_total"
adds segment_rank and segment_rank_sort (the STREAM class's, or in sort mode every
segment's, sorts).  The two paths' ranks and scores are compared byte for byte.

usage: local_probe.py GRAPH [REPS] [OUT.json] [shuffled]
GRAPH: roman (the full Roman-like graph), rmatK (R-MAT scale K, edge factor 8);
shuffled: the columns in random order (an unsorted src)"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "gnn-sparsification-research_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gsparse import graphs  # noqa: E402
from gsparse._lib import Context  # noqa: E402
from gsparse.engine import Engine  # noqa: E402

HBM_BYTES_PER_S = 6.29e12
WARM = 3

name = sys.argv[1] if len(sys.argv) > 1 else "roman"
reps = max(10, int(sys.argv[2])) if len(sys.argv) > 2 else 20
out_path = sys.argv[3] if len(sys.argv) > 3 else None
shuffle = len(sys.argv) > 4 and sys.argv[4] == "shuffled"

if name == "roman":
    ei, n = graphs.roman_like(), 22662
else:
    scale = int(name[4:])
    ei, n = graphs.rmat(scale, 8, seed=0), 1 << scale
ei = np.ascontiguousarray(ei, dtype=np.int64)
E = int(ei.shape[1])
rng = np.random.default_rng(0)
if shuffle:
    ei = np.ascontiguousarray(ei[:, rng.permutation(E)])
deg = np.bincount(ei[0], minlength=n)

ctx = Context(0)
ctx.set_graph_csr(2, np.array([0, 1, 2]), np.array([1, 0], dtype=np.int32), None)
eng = Engine(ctx)
t = torch.from_numpy(ei).cuda()
# a similarity-like score with ties: the two ends' degrees
s = torch.from_numpy((deg[ei[0]] + deg[ei[1]]).astype(np.float64)).cuda()
out = torch.empty(E, dtype=torch.float64, device="cuda")
res = {"graph": name, "nodes": n, "E": E, "reps": reps, "shuffled": shuffle, "max_degree": int(deg.max()),
       "src_sorted": bool((np.diff(ei[0]) >= 0).all())}

UNITS = ("segment_rank", "segment_rank_sort", "undirected_keys", "undirected_sort", "undirected_scan",
         "undirected_scatter", "local_scores")


def one(mode):
    if mode == "sort":
        os.environ["GSPARSE_SEGR_MODE"] = "sort"
    else:
        os.environ.pop("GSPARSE_SEGR_MODE", None)
    ctx.profile_reset()
    _, info = eng.local_scores(s, t[0], t[1], n, out=out)
    prof = ctx.profile_read()
    return {k: (prof[k]["ms"], prof[k]["bytes"]) for k in UNITS if k in prof}, info


ctx.profile(True)
runs = {"default": [], "sort": []}
for i in range(WARM + reps):
    for mode in ("default", "sort"):  # alternating: both see the same machine
        p, info = one(mode)
        if i >= WARM:
            runs[mode].append(p)
        res.setdefault("classes", {})[mode] = info["classes"]
ctx.profile(False)
os.environ.pop("GSPARSE_SEGR_MODE", None)

for mode, ps in runs.items():
    table = {}
    keys = sorted({k for p in ps for k in p})
    series = {k: [p.get(k, (0.0, 0.0))[0] for p in ps] for k in keys}
    nbytes = {k: max(p.get(k, (0.0, 0.0))[1] for p in ps) for k in keys}
    series["rank_total"] = [a + b for a, b in zip(series.get("segment_rank", [0.0] * len(ps)),
                                                  series.get("segment_rank_sort", [0.0] * len(ps)))]
    nbytes["rank_total"] = nbytes.get("segment_rank", 0.0) + nbytes.get("segment_rank_sort", 0.0)
    for k, v in series.items():
        med = statistics.median(v)
        table[k] = {"median_ms": med, "min_ms": min(v), "max_ms": max(v), "bytes": nbytes[k],
                    "GBps": nbytes[k] / 1e9 / (med / 1e3) if med > 0 else None,
                    "hbm_fraction": nbytes[k] / (med / 1e3) / HBM_BYTES_PER_S if med > 0 else None}
    res[mode] = table
res["sort_over_default_rank_total"] = res["sort"]["rank_total"]["median_ms"] / res["default"]["rank_total"]["median_ms"]

# the two paths give the same bytes
rd = eng.segment_rank(s, t[0], n)[0].cpu().numpy()
ld = eng.local_scores(s, t[0], t[1], n)[0].cpu().numpy()
os.environ["GSPARSE_SEGR_MODE"] = "sort"
rs = eng.segment_rank(s, t[0], n)[0].cpu().numpy()
ls = eng.local_scores(s, t[0], t[1], n)[0].cpu().numpy()
del os.environ["GSPARSE_SEGR_MODE"]
assert rd.tobytes() == rs.tobytes() and ld.tobytes() == ls.tobytes(), "the two paths differ"
res["paths_equal"] = True
print(json.dumps(res), flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
