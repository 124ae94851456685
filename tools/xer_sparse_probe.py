"""GPU box: the exact effective resistance (Engine.exact_er) on the largest component of
one graph, sparse form and -- up to 32768 nodes -- dense form.

CASE: rmat16 | rmat18 (R-MAT), arxiv (the ogbn-arxiv stand-in, citation_like), cora
(Cora-size Chung-Lu), roman (Roman-like, n = 22,662).

Per batch width of the sparse form (BATCHES: comma-separated GSPARSE_XER_BATCH values,
"default" for the plan's own): REPS timed calls with the graph resident (the call returns a
host array, so it is synchronous; the first call also pays the allocations and is reported
apart), the batches and the CG iterations of all columns; then one call under the context
profiler: the time in the Laplacian apply, in the vector passes and in the read-out, and
from them the apply's share.  REPS = 0: only the profiled call, whose wall time is then
the one reported (for graphs where a call takes minutes).  Foster's theorem (sum of
w_e R_e over the undirected edges = n - 1 on a connected graph) checks every result; below
the limit the dense form's scores do too.

usage: xer_sparse_probe.py CASE [OUT.json] [REPS] [BATCHES]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "gnn-sparsification-research_amd"))
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
from scipy.sparse.csgraph import connected_components  # noqa: E402

CAPS = dict(cg_rtol=1e-12, cg_max_iter=5000)  # the defaults gs_exact_er uses above the limit


def build(case):
    from gsparse import graphs

    if case.startswith("rmat"):
        scale = int(case[4:])
        ei, n = graphs.rmat(scale, 8, seed=0), 1 << scale
    elif case == "arxiv":
        ei, n = graphs.citation_like(), 169_343
    elif case == "cora":
        ei, n = graphs.chung_lu(), 2_708
    elif case == "roman":
        ei, n = graphs.roman_like(), 22_662
    else:
        raise SystemExit(__doc__)
    adj = sp.csr_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(n, n))
    _, lab = connected_components(adj, directed=False)
    nodes = np.flatnonzero(lab == np.argmax(np.bincount(lab)))
    sub = adj[nodes][:, nodes].tocsr()
    sub.sort_indices()
    return sub


def main():
    case = sys.argv[1] if len(sys.argv) > 1 else "rmat16"
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    batches = sys.argv[4].split(",") if len(sys.argv) > 4 else ["default"]

    import gsparse
    from gsparse._lib import Context
    from gsparse.engine import Engine, xer_sparse_plan

    sub = build(case)
    n = sub.shape[0]
    lens = np.diff(sub.indptr)
    rows = np.repeat(np.arange(n), lens)
    up = rows < sub.indices
    out = {"workload": f"exact effective resistance, largest component of {case}", "nodes": int(n),
           "entries": int(sub.nnz), "longest_row": int(lens.max()),
           "rows_split_into_segments": int((lens > 256).sum()), "reps": reps, "caps": CAPS,
           "forms": {}}

    ctx = Context()
    ctx.set_graph_csr(n, sub.indptr, sub.indices, sub.data)
    eng = Engine(ctx)

    def timed(call):
        t0 = time.perf_counter()
        v = call()
        return v, time.perf_counter() - t0

    dense = None
    if n <= 32768:
        rec = {}
        dense, rec["first_call_s"] = timed(lambda: eng.exact_er(method="dense"))
        ts = [timed(lambda: eng.exact_er(method="dense"))[1] for _ in range(max(reps, 1))]
        rec["median_s"], rec["min_s"] = statistics.median(ts), min(ts)
        rec["blocks"] = eng.exact_er_iterations
        rec["foster_rel_err"] = abs(float(np.sum(sub.data[up] * dense[up])) - (n - 1)) / (n - 1)
        out["forms"]["dense"] = rec
        print(json.dumps({"dense": rec}), flush=True)

    for b in batches:
        if b == "default":
            os.environ.pop("GSPARSE_XER_BATCH", None)
        else:
            os.environ["GSPARSE_XER_BATCH"] = b
        rec = {"batch": xer_sparse_plan(n)["batch"]}

        def call():
            return eng.exact_er(method="sparse", **CAPS)

        t0 = time.perf_counter()
        try:
            if reps > 0:
                er, rec["first_call_s"] = timed(call)
                ts = []
                for _ in range(reps):
                    again, s = timed(call)
                    ts.append(s)
                    assert np.array_equal(er.view(np.uint64), again.view(np.uint64)), "two calls differ"
                rec["median_s"], rec["min_s"], rec["max_s"] = statistics.median(ts), min(ts), max(ts)
            ctx.profile(True)
            ctx.profile_reset()
            er, rec["profiled_call_s"] = timed(call)
            prof = ctx.profile_read()
            ctx.profile(False)
            rec["batches"] = eng.exact_er_iterations
            rec["cg_iterations"] = eng.exact_er_cg_iterations
            ms = {k[len("xer_sparse_"):]: v["ms"] for k, v in prof.items() if k.startswith("xer_sparse_")}
            rec["profiled_ms"] = ms
            rec["batch_iterations"] = prof.get("xer_sparse_apply", {}).get("launches", 0)
            its = max(1, rec["batch_iterations"])
            rec["us_per_batch_iteration"] = 1e3 * (ms.get("apply", 0.0) + ms.get("vector", 0.0)) / its
            rec["us_per_column_iteration_wall"] = 1e6 * rec.get("median_s", rec["profiled_call_s"]) / max(
                1, rec["cg_iterations"])
            rec["apply_share"] = ms.get("apply", 0.0) / max(1e-30, ms.get("apply", 0.0) + ms.get("vector", 0.0))
            rec["foster_rel_err"] = abs(float(np.sum(sub.data[up] * er[up])) - (n - 1)) / (n - 1)
            if dense is not None:
                rec["max_rel_diff_to_dense"] = float(np.max(np.abs(er - dense) / dense))
        except gsparse.GsparseNotConverged as e:
            rec["not_converged"] = str(e)
            rec["failed_after_s"] = time.perf_counter() - t0
        out["forms"][f"sparse_B{rec['batch']}"] = rec
        print(json.dumps({f"sparse_B{rec['batch']}": rec}), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
