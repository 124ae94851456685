"""Wall time of the sampled selection: selection.sampled_mask_device (the rounds of
Generator.choice on the MI355X) against selection.sampled_mask (the reference's own
call on the host) on the same scores, with the device side's per-kernel split
(prep + total, ordered cumsum, divide, draw/search; per round) from the context's
event profile.  One JSON line per case.

  python tools/time_sampled.py                      # Roman size (r = 0.9, 0.2), 2^20 (r = 0.6)
  python tools/time_sampled.py --case 200000:0.5    # E:retention, repeatable
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "gnn-sparsification-research_amd"))
import gsparse  # noqa: E402
from gsparse.selection import sampled_mask, sampled_mask_device  # noqa: E402

DEFAULT_CASES = ["65854:0.9", "65854:0.2", f"{1 << 20}:0.6"]


def scores_for(E, seed=1):
    g = np.random.default_rng(seed)
    s = g.random(E)
    s[g.random(E) < 0.4] = 0.0  # the 1e-8 floor in play, as on sparse similarity scores
    return s


def best_of(fn, reps):
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        best = min(best, time.perf_counter() - t)
    return best, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--case", action="append", help="E:retention (default: %s)" % DEFAULT_CASES)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()

    ctx = gsparse._lib.Context()
    ctx.set_graph_csr(2, np.array([0, 1, 2]), np.array([1, 0], dtype=np.int32), None)
    eng = gsparse.engine.Engine(ctx)
    for case in args.case or DEFAULT_CASES:
        E, r = case.split(":")
        E, r = int(E), float(r)
        s = scores_for(E)
        info = {}
        sampled_mask_device(eng, s, E, r, args.seed, info=info)  # buffers, code loading
        t_dev, m_dev = best_of(lambda: sampled_mask_device(eng, s, E, r, args.seed), args.reps)
        t_host, m_host = best_of(lambda: sampled_mask(s, E, r, args.seed), max(1, args.reps // 2))
        ctx.profile(True)
        ctx.profile_reset()
        sampled_mask_device(eng, s, E, r, args.seed)
        prof = ctx.profile_read()
        ctx.profile(False)
        rounds = max(info["rounds"], 1)
        ms = {k: prof.get(k, {}).get("ms", 0.0) for k in
              ("sample_probs", "sample_cumsum", "sample_divide", "sample_draw")}
        print(json.dumps({
            "E": E, "retention": r, "seed": args.seed, "path": info["path"],
            "rounds": info["rounds"], "draws": info["draws"], "same_mask": bool(np.array_equal(m_dev, m_host)),
            "device_ms": round(t_dev * 1e3, 3), "host_ms": round(t_host * 1e3, 3),
            "prep_total_ms": round(ms["sample_probs"], 4),
            "cumsum_ms_per_round": round(ms["sample_cumsum"] / rounds, 4),
            "cumsum_ns_per_element": round(ms["sample_cumsum"] / rounds / E * 1e6, 3),
            "divide_ms_per_round": round(ms["sample_divide"] / rounds, 4),
            "draw_search_ms_per_round": round(ms["sample_draw"] / rounds, 4),
            "kernels_ms": round(sum(ms.values()), 3)}))


if __name__ == "__main__":
    main()
