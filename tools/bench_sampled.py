"""One epoch of neighbour-sampled mini-batch training (bot_amd.workloads.build_sampled) on one GPU, with its time split four ways:

  sample     sampling + block construction of every layer (csrc/sampling.hip, the blocks' row plans; includes the
             sampler's own device->host reads: the sampled total, the number of new sources and the CSC row pointer, per layer)
  gather     the gathers of the batch's node features (blocks[0].srcdata, with S-arxiv's label columns) and edge features (every
             block's edata)
  compute    forward + backward + optimizer step (the CSR of each block, built lazily in the backward, is counted here)
  sync       the host read of the batch loss (the reference's loss.item())

Each part ends in a device synchronise, so the parts add up to the epoch time.  One untimed warm-up batch comes first.
Prints one JSON line per workload (and writes them to --out): seeds/s, sampled edge-layers/s and the split.  With --prob the
in-edges are drawn in proportion to the workload's own edge weights (bot_amd.workloads.sampled_edge_weight: S-proteins the mean
of the 8 edge features, S-products a seeded uniform (0, 1] column); the one-off preparation of the weights happens in the
untimed warm-up batch and is reported on its own as "prepare_ms".

    python tools/bench_sampled.py [--workloads products proteins arxiv reddit cora] [--scale 1.0] [--prob] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def run(name, scale, seed, max_batches=None, prob=False):
    from bot_amd import workloads
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    t0 = time.perf_counter()
    wl = workloads.build_sampled(name, dev, scale=scale, seed=seed, prob=True if prob else None)
    torch.cuda.synchronize()
    t_build = time.perf_counter() - t0
    t_prep = None
    if prob:   # the one-off preparation, timed apart (the warm-up batch then finds it cached)
        from bot_amd import sampling
        t = time.perf_counter()
        sampling._prepared_weights(wl.graph, wl.loader.sampler.prob)
        torch.cuda.synchronize()
        t_prep = time.perf_counter() - t
    ef = name == "proteins"

    def batch(it, parts, counts):
        t = time.perf_counter()
        input_nodes, output_nodes, blocks = next(it)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        wl.inputs(blocks)
        if ef:
            for b in blocks:
                b.edata["feat"]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        loss = wl.step(blocks, output_nodes)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        float(loss.detach())
        t4 = time.perf_counter()
        for k, v in zip(("sample", "gather", "compute", "sync"), (t1 - t, t2 - t1, t3 - t2, t4 - t3)):
            parts[k] += v
        counts["seeds"] += int(output_nodes.numel())
        counts["edge_layers"] += sum(b.number_of_edges() for b in blocks)
        counts["sources_layer0"] = max(counts["sources_layer0"], blocks[0].number_of_src_nodes())
        counts["batches"] += 1

    warm = {k: 0.0 for k in ("sample", "gather", "compute", "sync")}
    batch(iter(wl.loader), warm, {"seeds": 0, "edge_layers": 0, "sources_layer0": 0, "batches": 0})
    parts = {k: 0.0 for k in warm}
    counts = {"seeds": 0, "edge_layers": 0, "sources_layer0": 0, "batches": 0}
    it = iter(wl.loader)
    n = len(wl.loader) if max_batches is None else min(max_batches, len(wl.loader))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        batch(it, parts, counts)
    total = time.perf_counter() - t0
    return {
        "workload": name, "scale": scale, "prob": bool(prob), "describe": wl.describe, "build_seconds": round(t_build, 2),
        "prepare_ms": None if t_prep is None else round(1e3 * t_prep, 2),
        "batches": counts["batches"], "epoch_seconds": round(total, 4), "ms_per_batch": round(1e3 * total / max(1, counts["batches"]), 3),
        "split_ms": {k: round(1e3 * v, 2) for k, v in parts.items()},
        "split_share": {k: round(v / total, 4) for k, v in parts.items()},
        "seeds_per_s": round(counts["seeds"] / total, 1), "sampled_edge_layers_per_s": round(counts["edge_layers"] / total, 1),
        "sampled_edge_layers": counts["edge_layers"], "max_sources_layer0": counts["sources_layer0"],
        "peak_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2), "device": torch.cuda.get_device_name(0),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["products", "proteins"])
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-batches", type=int, default=None, help="time only the first N batches of the epoch (profiling runs)")
    ap.add_argument("--prob", action="store_true", help="edge-weighted sampling with the workload's own weights")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sampled.py measures on an MI355X: no GPU here")
    lines = []
    for name in a.workloads:
        r = run(name, a.scale, a.seed, a.max_batches, a.prob)
        print(json.dumps(r), flush=True)
        lines.append(r)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
