"""The timed subgraph batch that tools/bench_clustered.py (epoch leg) and tools/bench_saint.py share."""
import time

import torch

STAGES = ("extract", "plan", "gather", "compute")


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def timed_batch(wl, nodes, edge_feat=False, t0=None):
    """One train step of `wl` (a workloads.SubgraphWorkload) on the batch the node set `nodes` induces, each of STAGES ending in a
    device synchronise so that they add up: ({stage: seconds}, {"nodes", "edges", "skipped"} of the batch, the Subgraph).  `t0`: the
    synchronised time at which the caller's own previous stage ended, where it has one (no second synchronise, no gap)."""
    from bot_amd import _C
    from bot_amd.sampling import Subgraph, _node_map
    g = wl.graph
    if t0 is None:
        t0 = sync()
    arrays = _C.node_subgraph(g.csc, nodes, _node_map(g))
    t1 = sync()
    sub = Subgraph(g, nodes, *arrays)
    _ = sub.csr, sub.csr2csc
    t2 = sync()
    sub.ndata["feat"]
    if edge_feat:
        sub.edata["feat"]
    t3 = sync()
    out = wl.step(sub)
    if out is not None:
        float(out[0].detach())
    t4 = sync()
    counts = {"nodes": sub.number_of_nodes(), "edges": sub.number_of_edges(), "skipped": int(out is None)}
    return dict(zip(STAGES, (t1 - t0, t2 - t1, t3 - t2, t4 - t3))), counts, sub
