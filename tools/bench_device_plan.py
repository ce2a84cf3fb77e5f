"""Construction of a mini-batch graph on one GPU: the device path (csrc/plan.hip: row plans and the CSC transpose on the device)
against the host path of the same commit (`graph.DEVICE_PLAN = False`: the host planner and `graph.build_direction`), alternating
in one process.

Per leg (`family:workload`, a child process of its own under a time limit; the first one that fails or runs out of time ends the
run) the batches of an epoch are produced as usual (samplers / walks / extraction: not timed), and for every batch the construction
up to a finished CSC plan + CSR + CSR plan + csr2csc is timed under both settings, between device synchronises, the setting that
goes first alternating from batch to batch.  A sampled batch is its list of blocks (one construction per layer, summed).  Three
rounds; per round the median over the epoch's batches; reported: the median of the rounds and their spread (largest minus
smallest round) for each path, and whether the device path beats the host path by more than the host path's own spread.

    python tools/bench_device_plan.py [--legs sampled:products sampled:arxiv clustered:arxiv ...] [--scale 1.0] [--rounds 3]
                                      [--max-batches N] [--out profiles/bench_device_plan.jsonl]

The kernels' own durations: one `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_device_plan.py --child
clustered:arxiv --rounds 1` run (no counters in that run); its kernel statistics are profiles/bench_device_plan_kernel_stats.csv.
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import torch  # noqa: E402

LEGS = ["sampled:products", "sampled:arxiv", "clustered:arxiv", "clustered:reddit", "clustered:products", "saint:arxiv", "saint:reddit",
        "saint:products"]


def _sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def _batches(family, wl, max_batches):
    """The epoch's batches as lists of constructor arguments: [(class, args)] per batch (a sampled batch: one entry per block)."""
    from bot_amd import _C
    from bot_amd.sampling import Block, Subgraph, _draw_seed, _node_map, _prepared_weights
    g = wl.graph
    if family == "sampled":
        loader = wl.loader
        n = int(loader.nids.numel())
        order = torch.randperm(n, generator=loader.generator).to(loader.nids.device)
        for b in range(len(loader)):
            if max_batches is not None and b >= max_batches:
                return
            seeds = loader.nids[order[b * loader.batch_size:(b + 1) * loader.batch_size]].to(torch.int32).contiguous()
            out = []
            for fanout in reversed(loader.sampler.fanouts):
                seed = _draw_seed(loader.generator)
                if loader.sampler.prob is None:
                    offsets, pos = _C.sample_neighbors(g.csc, seeds, fanout, seed)
                else:
                    offsets, pos = _C.sample_neighbors_weighted(g.csc, _prepared_weights(g, loader.sampler.prob), seeds, fanout, seed)
                src_nid, local, parent_eid = _C.block_relabel(g.csc, seeds, pos, _node_map(g))
                out.insert(0, (Block, (g, src_nid, offsets, local, parent_eid)))
                seeds = src_nid
            yield out
    else:
        for b, nodes in enumerate(wl.loader.node_batches()):
            if max_batches is not None and b >= max_batches:
                return
            yield [(Subgraph, (g, nodes) + tuple(_C.node_subgraph(g.csc, nodes, _node_map(g))))]


def _construct(G, batch, flag):
    G.DEVICE_PLAN = flag
    t0 = _sync()
    graphs = [cls(*args) for cls, args in batch]
    for b in graphs:
        _ = b.csr, b.csr2csc
    return _sync() - t0, graphs


def child(leg, a):
    from bot_amd import _C, workloads
    G = importlib.import_module("bot_amd.graph")
    family, name = leg.split(":")
    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    build = {"sampled": workloads.build_sampled, "clustered": workloads.build_clustered, "saint": workloads.build_saint}[family]
    wl = build(name, dev, scale=a.scale, seed=a.seed)
    g = wl.graph
    for batch in _batches(family, wl, 1):                        # warm-up: one batch under each setting
        _construct(G, batch, True), _construct(G, batch, False)
    rounds = {"device": [], "host": []}
    edges = nodes = count = 0
    c0 = dict(_C.PLAN_COUNTS)
    for _ in range(a.rounds):
        per = {"device": [], "host": []}
        for i, batch in enumerate(_batches(family, wl, a.max_batches)):
            for flag in ((True, False) if i % 2 == 0 else (False, True)):      # alternating
                seconds, graphs = _construct(G, batch, flag)
                per["device" if flag else "host"].append(seconds)
            edges += sum(b.number_of_edges() for b in graphs)
            nodes += sum(b.number_of_src_nodes() for b in graphs)
            count += 1
        for k in per:
            rounds[k].append(round(1e3 * statistics.median(per[k]), 4))
    G.DEVICE_PLAN = True
    out = {"leg": leg, "scale": a.scale, "n_nodes": g.number_of_nodes(), "n_edges": g.number_of_edges(), "batches_per_round": count // max(a.rounds, 1),
           "graphs_per_batch": len(batch), "src_nodes_per_batch": nodes // max(count, 1), "edges_per_batch": edges // max(count, 1),
           "plan_counts": {k: _C.PLAN_COUNTS[k] - c0[k] for k in c0}, "device": torch.cuda.get_device_name(0)}
    for k in rounds:
        out[k + "_ms_rounds"] = rounds[k]
        out[k + "_ms_median"] = round(statistics.median(rounds[k]), 4)
        out[k + "_ms_spread"] = round(max(rounds[k]) - min(rounds[k]), 4)
    out["device_beats_host_by_more_than_host_spread"] = out["host_ms_median"] - out["device_ms_median"] > out["host_ms_spread"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="+", default=LEGS)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-batches", type=int, default=None, help="time only the first N batches of an epoch")
    ap.add_argument("--timeout", type=int, default=420, help="seconds a leg's child process may run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_device_plan.jsonl"))
    ap.add_argument("--child", metavar="LEG", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        if not torch.cuda.is_available():
            sys.exit("bench_device_plan.py measures on an MI355X: no GPU here")
        print("RESULT " + json.dumps(child(a.child, a)), flush=True)
        return
    passed, skip = [], False
    for x in sys.argv[1:]:                                       # the child's arguments: everything but --legs and its values
        if x == "--legs":
            skip = True
        elif x.startswith("--"):
            skip = False
        if not skip:
            passed.append(x)
    with open(a.out, "a") as f:
        for leg in a.legs:
            cmd = [sys.executable, os.path.abspath(__file__)] + passed + ["--child", leg]
            try:
                out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                sys.exit(f"{leg}: no result within {a.timeout} s; stopping here")
            lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
            if out.returncode != 0 or not lines:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                sys.exit(f"{leg}: child ended with rc {out.returncode}; stopping here")
            print(lines[-1][7:], flush=True)
            f.write(lines[-1][7:] + "\n")
            f.flush()


if __name__ == "__main__":
    main()
