"""GraphSAINT mini-batch training (bot_amd.workloads.build_saint) on one GPU, measured beside the cluster batches it is an
alternative to.  Every workload runs in a child process of its own under a time limit; the first one that fails or runs out of
time ends the run (nothing more is started on the GPU after a fault).

Per workload one child process builds `build_saint(name)` and `build_clustered(name)` and runs their epochs ALTERNATING (SAINT,
clustered, SAINT, ...), `--rounds` of each, so that the edges-per-batch comparison is measured where the timing is.  Per epoch (or
--max-batches of it) the time of a batch is split five ways, each part ending in a device synchronise so that the parts add up:
  nodes     SAINT: bot_saint_walk + bot_saint_nodes_mark / list and the one device->host read (the node count);
            clustered: the loader's part lookup
  extract   bot_subgraph_mark / count / fill / unmark, the scan of the counts and the one device->host read
  plan      the Subgraph object: row plan of the CSC (host), and the CSR + csr2csc (graph.build_direction)
  gather    the batch's node features (and edge features, S-proteins) out of the parent's frames
  compute   forward + backward + optimizer step (train.train_step, or model(sub) + the node loss) and the loss read
plus nodes, edges and edges that are not self-loops per batch, the peak allocated bytes of each side's epochs, and for SAINT the
one-off pre-sampling time of the loss weights (saint_loss_weights inside build_saint).  Medians over the rounds, and their spread.

--aggregator-norm (the GCN recipes: S-reddit by default): one child builds `build_saint(name, aggregator_norm=True)` and the plain
`build_saint(name)` and runs their epochs alternating, `--rounds` of each: ms per batch with and without GraphSAINT's per-edge
aggregator normalisation (the gather of the batch's rows of the column and the weighted SpMMs fall into `compute`), and the one-off
pre-sampling time of `saint_norms` beside `saint_loss_weights`; into profiles/bench_saint_norm.jsonl.

    python tools/bench_saint.py [--workloads arxiv reddit products] [--mode walk] [--scale 1.0] [--rounds 3] [--out profiles/bench_saint.jsonl]

The walk kernel's own duration: one `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_saint.py --child arxiv
--rounds 1` run (no counters in that run); its kernel statistics are profiles/bench_saint_kernel_stats.csv.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import torch  # noqa: E402
from subgraph_batch import STAGES, sync as _sync, timed_batch  # noqa: E402

KEYS = ("nodes",) + STAGES


def _epoch(wl, name, max_batches):
    """One epoch of `wl` (a workloads.SubgraphWorkload) with the batch time split by KEYS."""
    parts = {k: 0.0 for k in KEYS}
    c = {"nodes": 0, "edges": 0, "non_loop_edges": 0, "skipped": 0, "batches": 0}
    torch.cuda.reset_peak_memory_stats()
    it = iter(wl.loader.node_batches())
    while max_batches is None or c["batches"] < max_batches:
        t = _sync()
        nodes = next(it, None)
        if nodes is None:
            break
        t0 = _sync()
        parts["nodes"] += t0 - t
        seconds, counts, sub = timed_batch(wl, nodes, edge_feat=name == "proteins", t0=t0)
        s, d = sub.edges()                                      # (counted outside the timed parts)
        for k, v in seconds.items():
            parts[k] += v
        for k, v in counts.items():
            c[k] += v
        c["non_loop_edges"] += int((s != d).sum())
        c["batches"] += 1
    total = sum(parts.values())                                 # the parts are contiguous: they add up to the batch
    b = max(1, c["batches"])
    return {"ms_per_batch": round(1e3 * total / b, 3), "split_ms_per_batch": {k: round(1e3 * v / b, 3) for k, v in parts.items()},
            "batches": c["batches"], "skipped": c["skipped"], "nodes_per_batch": c["nodes"] // b, "edges_per_batch": c["edges"] // b,
            "non_loop_edges_per_batch": c["non_loop_edges"] // b, "peak_allocated_bytes": int(torch.cuda.max_memory_allocated())}


def _summary(rounds):
    ms = [r["ms_per_batch"] for r in rounds]
    out = {"rounds": rounds, "ms_per_batch_median": round(statistics.median(ms), 3), "ms_per_batch_spread": round(max(ms) - min(ms), 3),
           "split_ms_per_batch_median": {k: round(statistics.median([r["split_ms_per_batch"][k] for r in rounds]), 3) for k in KEYS}}
    for k in ("nodes_per_batch", "edges_per_batch", "non_loop_edges_per_batch", "peak_allocated_bytes"):
        out[k + "_median"] = int(statistics.median([r[k] for r in rounds]))
    return out


def child(name, a):
    from bot_amd import workloads
    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    t0 = time.perf_counter()
    saint = workloads.build_saint(name, dev, scale=a.scale, seed=a.seed, mode=a.mode, length=a.length)
    t_saint = _sync() - t0
    clustered = workloads.build_clustered(name, dev, scale=a.scale, seed=a.seed)
    g = saint.graph
    for wl in (saint, clustered):                                # warm-up: one batch each
        _epoch(wl, name, 1)
    rounds = {"saint": [], "clustered": []}
    for _ in range(a.rounds):                                    # alternating
        rounds["saint"].append(_epoch(saint, name, a.max_batches))
        rounds["clustered"].append(_epoch(clustered, name, a.max_batches))
    return {"workload": name, "scale": a.scale, "mode": a.mode, "describe": saint.describe, "n_nodes": g.number_of_nodes(),
            "n_edges": g.number_of_edges(), "budget": saint.loader.sampler.budget, "n_batches": len(saint.loader),
            "presample_sets": workloads.saint_defaults(name, g.number_of_nodes(), mode=a.mode, length=a.length)[2],
            "presample_seconds": round(saint.presample_s, 3), "build_saint_seconds": round(t_saint, 2),
            "saint": _summary(rounds["saint"]), "clustered": _summary(rounds["clustered"]), "device": torch.cuda.get_device_name(0)}


def child_norm(name, a):
    from bot_amd import workloads
    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    kw = dict(scale=a.scale, seed=a.seed, mode=a.mode, length=a.length)
    plain = workloads.build_saint(name, dev, **kw)
    normed = workloads.build_saint(name, dev, aggregator_norm=True, **kw)
    g = normed.graph
    en = g.edata[workloads.SAINT_NORM]
    for wl in (normed, plain):                                   # warm-up: one batch each
        _epoch(wl, name, 1)
    rounds = {"aggregator_norm": [], "plain": []}
    for _ in range(a.rounds):                                    # alternating
        rounds["aggregator_norm"].append(_epoch(normed, name, a.max_batches))
        rounds["plain"].append(_epoch(plain, name, a.max_batches))
    return {"workload": name, "scale": a.scale, "mode": a.mode, "describe": normed.describe, "n_nodes": g.number_of_nodes(),
            "n_edges": g.number_of_edges(), "budget": normed.loader.sampler.budget, "n_batches": len(normed.loader),
            "presample_sets": workloads.saint_defaults(name, g.number_of_nodes(), mode=a.mode, length=a.length)[2],
            "saint_loss_weights_seconds": round(plain.presample_s, 3), "saint_norms_seconds": round(normed.presample_s, 3),
            "edge_norm_max": float(en.max()), "edge_norm_mean": round(float(en.mean()), 4), "edges_never_induced": int((en == 1.0).sum()),
            "aggregator_norm": _summary(rounds["aggregator_norm"]), "plain": _summary(rounds["plain"]),
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=None, help="default arxiv reddit products (reddit with --aggregator-norm)")
    ap.add_argument("--aggregator-norm", action="store_true", help="ms per batch with and without the aggregator normalisation")
    ap.add_argument("--mode", default="walk", choices=["walk", "node"])
    ap.add_argument("--length", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-batches", type=int, default=None, help="time only the first N batches of an epoch")
    ap.add_argument("--timeout", type=int, default=420, help="seconds a workload's child process may run")
    ap.add_argument("--out", default=None, help="default profiles/bench_saint.jsonl (bench_saint_norm.jsonl with --aggregator-norm)")
    ap.add_argument("--child", metavar="WORKLOAD", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        if not torch.cuda.is_available():
            sys.exit("bench_saint.py measures on an MI355X: no GPU here")
        print("RESULT " + json.dumps((child_norm if a.aggregator_norm else child)(a.child, a)), flush=True)
        return
    if a.workloads is None:
        a.workloads = ["reddit"] if a.aggregator_norm else ["arxiv", "reddit", "products"]
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "bench_saint_norm.jsonl" if a.aggregator_norm else "bench_saint.jsonl")
    passed = [x for x in sys.argv[1:]]
    with open(a.out, "a") as f:
        for name in a.workloads:
            cmd = [sys.executable, os.path.abspath(__file__)] + passed + ["--child", name]
            try:
                out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                sys.exit(f"{name}: no result within {a.timeout} s; stopping here")
            lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
            if out.returncode != 0 or not lines:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                sys.exit(f"{name}: child ended with rc {out.returncode}; stopping here")
            print(lines[-1][7:], flush=True)
            f.write(lines[-1][7:] + "\n")
            f.flush()


if __name__ == "__main__":
    main()
