"""GPU box: what the trussness (gs_trussness) costs against its own support pass
(gs_common_neighbors, the counts the peel starts from), on one graph resident on the
device, and what the tail cap GSPARSE_TRUSS_TAIL does to it.

After one warm-up of each, REPS (>= 5) rounds in which gs_common_neighbors and
gs_trussness under every cap of CAPS (0 = no tail) are timed one after the other, so that
the forms alternate; the host clock around a call that ends in a stream synchronise; the
medians and the minima are reported, with the levels, sub-rounds, host waits and largest
trussness under every cap, and the ratio of each median to the support pass's.  The
scores of every cap must be the same bytes.

With SAVE the trussness (uint16, CSR order) is written to SAVE (.npz) with the graph's
name; on any machine,
  truss_probe.py --verify SAVE
then builds the same graph again and checks the scores without a specification: for every
k present, every kept entry of {t >= k} lies in at least k - 2 triangles of that subgraph
(a sparse product on the host, in row blocks).

usage: truss_probe.py GRAPH [REPS] [OUT.json] [CAPS=0,256,4096,65536] [SAVE.npz]
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
import scipy.sparse as sp  # noqa: E402


def graph(name):
    from gsparse import graphs

    if name == "roman":
        return graphs.roman_like(), 22662
    if name == "citation":
        return graphs.citation_like(), 169343
    scale = int(name[4:])
    return graphs.rmat(scale, 8, seed=0), 1 << scale


def verify(path, block=8192):
    z = np.load(path)
    t = z["t"].astype(np.int64)
    ei, n = graph(str(z["graph"]))
    a = sp.csr_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(n, n))
    a.sum_duplicates()
    a.sort_indices()
    ip, ix = a.indptr, a.indices
    assert len(ix) == len(t), "the scores are not this graph's"
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ip))
    assert (t[rows == ix] == 0).all() and (t[rows != ix] >= 2).all()
    ks = np.unique(t[t > 0])
    worst = {}
    for k in ks.tolist():
        keep = t >= k
        a = sp.csr_matrix((np.ones(int(keep.sum()), dtype=np.int32), (rows[keep], ix[keep])), shape=(n, n))
        lo = np.iinfo(np.int64).max
        for r0 in range(0, n, block):
            blk = a[r0:r0 + block]
            if blk.nnz == 0:
                continue
            tri = (blk @ a).multiply(blk).tocsr()
            # an entry in no triangle is no stored entry of the product
            lo = min(lo, int(tri.data.min()) if tri.nnz == blk.nnz else 0)
        worst[k] = lo
        assert lo >= k - 2, f"k = {k}: a kept entry lies in {lo} triangles of the subgraph"
    print(json.dumps({"verified": os.path.basename(path), "entries": int(len(t)), "levels": len(ks),
                      "max_truss": int(ks[-1]) if len(ks) else 0,
                      "least_support_per_k": {str(k): v for k, v in worst.items()}}))


if len(sys.argv) > 2 and sys.argv[1] == "--verify":
    verify(sys.argv[2])
    sys.exit(0)

import torch  # noqa: E402

from gsparse._lib import Context  # noqa: E402
from gsparse.engine import Engine  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "roman"
reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else None
caps = [int(x) for x in (sys.argv[4] if len(sys.argv) > 4 else "0,256,4096,65536").split(",")]
save = sys.argv[5] if len(sys.argv) > 5 else None

ei, n = graph(name)
ei = np.ascontiguousarray(ei, dtype=np.int64)

ctx = Context(0)
ctx.set_graph_edge_index(n, ei[0], ei[1])
eng = Engine(ctx)
nnz = eng.nnz
out = {"graph": name, "nodes": n, "entries": nnz, "reps": reps, "caps": caps}
buf = torch.empty(nnz, dtype=torch.float64, device="cuda")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def truss(cap):
    os.environ["GSPARSE_TRUSS_TAIL"] = str(cap)
    return eng.trussness(out=buf)[1]


eng.common_neighbors(out=buf)  # warm-up: the Jaccard plan, the code objects
want = None
for cap in caps:
    info = truss(cap)
    got = buf.cpu().numpy()
    if want is None:
        want, info0 = got, info
    assert got.tobytes() == want.tobytes(), f"cap {cap}: other scores"
    assert (info["levels"], info["rounds"], info["max_truss"]) == \
        (info0["levels"], info0["rounds"], info0["max_truss"]), (cap, info, info0)
    out[f"info_tail{cap}"] = info
ts = {"support": []}
ts.update({cap: [] for cap in caps})
for _ in range(reps):
    ts["support"].append(timed(lambda: eng.common_neighbors(out=buf))[0])
    for cap in caps:
        ts[cap].append(timed(lambda: truss(cap))[0])
sup = statistics.median(ts["support"])
out["support_s"], out["support_min_s"] = sup, min(ts["support"])
for cap in caps:
    med = statistics.median(ts[cap])
    out[f"truss_tail{cap}_s"], out[f"truss_tail{cap}_min_s"] = med, min(ts[cap])
    out[f"truss_tail{cap}_over_support"] = med / sup
out.update(levels=info0["levels"], rounds=info0["rounds"], max_truss=info0["max_truss"])
if save:
    assert want.max() < 65536
    np.savez_compressed(save, graph=name, t=want.astype(np.uint16))
print(json.dumps(out))
if out_path:
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
