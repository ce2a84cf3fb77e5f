"""Induced-subgraph (cluster) mini-batch training (bot_amd.workloads.build_clustered) on one GPU, measured three ways.  Every leg
runs in a child process of its own under a time limit; the first leg that fails or runs out of time ends the run (nothing more is
started on the GPU after a fault).

  epoch     per workload and round one epoch (or --max-batches of it) with the time of a batch split four ways, each part ending
            in a device synchronise so that the parts add up:
              extract   bot_subgraph_mark / count / fill / unmark, the scan of the counts and the one device->host read
              plan      the Subgraph object: row plan of the CSC (host), and the CSR + csr2csc (graph.build_direction)
              gather    the batch's node features (and edge features, S-proteins) out of the parent's frames
              compute   forward + backward + optimizer step (train.train_step, or model(sub) + the node loss) and the loss read
            plus nodes and edges per batch, the share of the parent's edges that survive inside the batches (parts_per_batch = 1)
            under "community" and under "random" parts, and the peak allocated bytes.
  full      the full-batch step of workloads.build(name): ms per step and peak allocated bytes, for the memory comparison.
  extract   the kernel against the construction available without it, alternating in one process: membership table + boolean mask
            over the parent's edge list + bot_amd.graph.graph on the kept edges, both timed up to a finished CSC with its row plan,
            over the node sets of one epoch; median per round, ratio and the rounds' spread.

    python tools/bench_clustered.py [--workloads arxiv reddit products] [--scale 1.0] [--rounds 3] [--out profiles/bench_clustered.jsonl]
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


def leg_epoch(name, a):
    from bot_amd import workloads
    from bot_amd.sampling import cluster_assignment
    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    t0 = time.perf_counter()
    wl = workloads.build_clustered(name, dev, scale=a.scale, seed=a.seed, method=a.method, parts_per_batch=a.parts_per_batch)
    t_build = _sync() - t0
    g = wl.graph
    gs, gd = g.edges()
    survive = {}
    n_parts = wl.loader.n_parts
    for method in ("community", "random"):
        parts = wl.parts if method == a.method else cluster_assignment(g, n_parts, method, a.seed)
        survive[method] = round(float((parts[gs] == parts[gd]).float().mean()), 4)
    ef = name == "proteins"
    timed_batch(wl, next(iter(wl.loader.node_batches())), ef)   # warm-up
    torch.cuda.reset_peak_memory_stats()
    rounds = []
    for _ in range(a.rounds):
        parts = {k: 0.0 for k in STAGES}
        counts = {"nodes": 0, "edges": 0, "skipped": 0, "batches": 0}
        t0 = _sync()
        for i, nodes in enumerate(wl.loader.node_batches()):
            if a.max_batches is not None and i >= a.max_batches:
                break
            seconds, one, _ = timed_batch(wl, nodes, ef)
            for k, v in seconds.items():
                parts[k] += v
            for k, v in one.items():
                counts[k] += v
            counts["batches"] += 1
        total = _sync() - t0
        b = max(1, counts["batches"])
        rounds.append({"ms_per_batch": round(1e3 * total / b, 3), "split_ms_per_batch": {k: round(1e3 * v / b, 3) for k, v in parts.items()},
                       "batches": counts["batches"], "skipped": counts["skipped"], "nodes_per_batch": counts["nodes"] // b,
                       "edges_per_batch": counts["edges"] // b})
    ms = [r["ms_per_batch"] for r in rounds]
    return {"leg": "epoch", "workload": name, "scale": a.scale, "method": a.method, "describe": wl.describe, "build_seconds": round(t_build, 2),
            "n_nodes": g.number_of_nodes(), "n_edges": g.number_of_edges(), "n_parts": n_parts, "parts_per_batch": a.parts_per_batch,
            "edge_share_inside_parts": survive, "rounds": rounds, "ms_per_batch_median": statistics.median(ms),
            "ms_per_batch_spread": round(max(ms) - min(ms), 3), "peak_allocated_bytes": int(torch.cuda.max_memory_allocated()),
            "device": torch.cuda.get_device_name(0)}


def leg_full(name, a):
    from bot_amd import workloads
    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    wl = workloads.build(name, dev, seed=a.seed, scale=a.scale)
    for _ in range(2):
        wl.step()
    torch.cuda.reset_peak_memory_stats()
    rounds = []
    for _ in range(a.rounds):
        t0 = _sync()
        for _ in range(a.full_steps):
            wl.step()
        rounds.append(round(1e3 * (_sync() - t0) / a.full_steps, 3))
    return {"leg": "full", "workload": name, "scale": a.scale, "ms_per_step_rounds": rounds, "ms_per_step_median": statistics.median(rounds),
            "peak_allocated_bytes": int(torch.cuda.max_memory_allocated()), "device": torch.cuda.get_device_name(0)}


def leg_extract(name, a):
    import bot_amd
    from bot_amd import synth, workloads
    from bot_amd.sampling import ClusterLoader, cluster_assignment
    dev = torch.device("cuda:0")
    edge = name in ("proteins", "products")
    ds = workloads._edge_dataset(name, dev, a.seed, a.scale) if edge else synth.make_dataset(name, device=dev, seed=a.seed, scale=a.scale)
    g = ds.graph
    n = g.number_of_nodes()
    n_parts = workloads.CLUSTERED[name]
    loader = ClusterLoader(g, cluster_assignment(g, n_parts, a.method, a.seed), parts_per_batch=a.parts_per_batch, seed=a.seed)
    gs, gd = g.edges()
    table = torch.full((n,), -1, dtype=torch.int64, device=dev)

    def by_kernel(nodes):
        sub = g.subgraph(nodes)                       # extraction + the CSC's row plan
        return sub.number_of_edges()

    def by_tensor_ops(nodes):
        idx = nodes.long()
        table[idx] = torch.arange(idx.numel(), device=dev)
        ls, ld = table[gs], table[gd]
        keep = (ls >= 0) & (ld >= 0)
        twin = bot_amd.graph((ls[keep], ld[keep]), num_nodes=int(idx.numel()))
        _ = twin.csc                                  # argsort by destination + the row plan
        table[idx] = -1
        return twin.number_of_edges()

    sets = [b.clone() for i, b in enumerate(loader.node_batches()) if a.max_batches is None or i < a.max_batches]
    assert by_kernel(sets[0]) == by_tensor_ops(sets[0])          # warm-up, and the two agree on the edge count
    rounds = []
    for _ in range(a.rounds):
        tk, tt = [], []
        for nodes in sets:                            # alternating, batch by batch
            t0 = _sync()
            by_kernel(nodes)
            t1 = _sync()
            by_tensor_ops(nodes)
            t2 = _sync()
            tk.append(t1 - t0)
            tt.append(t2 - t1)
        rounds.append({"kernel_ms": round(1e3 * statistics.median(tk), 3), "tensor_ops_ms": round(1e3 * statistics.median(tt), 3),
                       "ratio": round(statistics.median(tt) / statistics.median(tk), 3)})
    ratios = [r["ratio"] for r in rounds]
    return {"leg": "extract", "workload": name, "scale": a.scale, "method": a.method, "n_nodes": n, "n_edges": g.number_of_edges(),
            "n_parts": n_parts, "batches_timed": len(sets), "rounds": rounds, "ratio_median": statistics.median(ratios),
            "ratio_spread": round(max(ratios) - min(ratios), 3), "device": torch.cuda.get_device_name(0)}


LEGS = {"epoch": leg_epoch, "full": leg_full, "extract": leg_extract}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["arxiv", "reddit", "products"])
    ap.add_argument("--legs", nargs="+", default=["epoch", "extract", "full"], choices=list(LEGS))
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--method", default="community", choices=["community", "random"])
    ap.add_argument("--parts-per-batch", type=int, default=1)
    ap.add_argument("--max-batches", type=int, default=None, help="time only the first N batches of an epoch")
    ap.add_argument("--full-steps", type=int, default=5)
    ap.add_argument("--leg-timeout", type=int, default=420, help="seconds a leg's child process may run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_clustered.jsonl"))
    ap.add_argument("--child", nargs=2, metavar=("LEG", "WORKLOAD"), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        if not torch.cuda.is_available():
            sys.exit("bench_clustered.py measures on an MI355X: no GPU here")
        print("RESULT " + json.dumps(LEGS[a.child[0]](a.child[1], a)), flush=True)
        return
    passed = [x for x in sys.argv[1:]]
    with open(a.out, "a") as f:
        for name in a.workloads:
            for leg in a.legs:
                cmd = [sys.executable, os.path.abspath(__file__)] + passed + ["--child", leg, name]
                try:
                    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.leg_timeout)
                except subprocess.TimeoutExpired:
                    sys.exit(f"{leg} {name}: no result within {a.leg_timeout} s; stopping here")
                lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
                if out.returncode != 0 or not lines:
                    sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                    sys.exit(f"{leg} {name}: child ended with rc {out.returncode}; stopping here")
                print(lines[-1][7:], flush=True)
                f.write(lines[-1][7:] + "\n")
                f.flush()


if __name__ == "__main__":
    main()
